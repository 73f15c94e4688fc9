"""
Hyperparameters from the WHOLE of a large design: the Vecchia (nearest-neighbour) approximation of the Gaussian likelihood (Vecchia 1988;
Datta et al. 2016; Guinness 2018; Katzfuss et al. 2020, "scaled Vecchia"), evaluated with its analytic gradient on the device.

    log p(y) ~ sum_t log p(y_t | y_c(t)),     c(t) = the min(t, k) nearest points among those BEFORE t in an ordering

N independent problems of at most (k + 1) x (k + 1), k <= 126: an ordered neighbour search and one 128 x 128 factorisation per point
(``csrc/kernels_local.hip``), on the native handle ``LocalGP`` predicts from.  The design goes up once, in the Vecchia order, and serves the
fit and the prediction.

    r2(x, x') = sum_d exp(theta_d) (x_d - x'_d)^2            (one shared theta for the uniform kernels)
    A = sigma^2 k(r2) + (nugget + jitter) I over (c(t), t) = L L^T,   e the last row,   z = L^-1 y
    l_t = -log L_ee - z_e^2 / 2 - log(2 pi) / 2

theta is laid out as the package lays it out for a zero mean: the correlation raws (D of them, 1 for the uniform kernels), log sigma^2, and
log nugget with ``nugget="fit"``.  The neighbour search follows the contract of ``LocalGP``'s (one rounded multiply per coordinate, r2 summed
ascending in d without fused multiply-add, the smallest (r2, index) pairs, ties to the lowest position), so NumPy reproduces every list.
Value and gradient are summed without atomics in an order that depends on N alone: the same bits for a repeated call and any ``max_points``.

``loglik_exact`` and ``fit_exact`` evaluate and maximise the EXACT likelihood of the whole design on the same handle (``IterativeGP.py``:
one matrix-free CG solve and stochastic Lanczos quadrature per evaluation), typically started from the Vecchia optimum.

Not covered: priors, mean functions (the mean is zero), several outputs or several theta per call, a maximin ordering on the device,
grouped Vecchia, ``ProductMat52``, ``nugget="adaptive"`` / ``"pivot"``, k > 126, several devices.
"""
import numpy as np

from .IterativeGP import IterativeGP as _IterativeGP, _check_options, _check_probes, _exact_loglik
from .LocalGP import MAX_D, MAX_NEIGHBOURS, _KERNELS, LocalGP as _LocalGP, _create_native as _create_local_native

_FAILED = 1e30          # what the optimiser sees in place of a non-finite evaluation (with a zero gradient)


class VecchiaLogLik(object):
    """What ``VecchiaGP.loglik`` returns:

    * ``value``      the Vecchia log-likelihood; ``-inf`` when a local matrix was not positive definite
    * ``grad``       (P,) its gradient with respect to theta with ``grad=True`` (NaN when a point failed), else None
    * ``terms``      (N,) log p(y_t | y_c(t)) in the caller's numbering with ``return_terms=True`` (NaN where ``ok`` is False), else None
    * ``ok``         (N,) bool, the caller's numbering: the local matrix of that point was positive definite
    * ``n_failed``   the number of False flags in ``ok``"""

    def __init__(self, value, grad, terms, ok):
        self.value, self.grad, self.terms, self.ok = value, grad, terms, ok

    @property
    def n_failed(self):
        return int(np.size(self.ok) - np.count_nonzero(self.ok))


class VecchiaFit(object):
    """What ``VecchiaGP.fit`` returns, for the best try: ``theta``, ``value`` (the log-likelihood on the final neighbour lists), ``grad`` (its
    gradient there), ``n_evaluations``, ``n_refreshes`` (rebuilds of the lists that were followed by a resumed optimisation), ``converged``
    (every optimisation run of that try ended by one of L-BFGS-B's own rules, not by its iteration limit or a failed line search) and
    ``tries``: per try a dict with ``theta0``, ``start_value``, ``theta``, ``value``, ``grad``, ``n_evaluations``, ``n_refreshes``,
    ``converged``, ``message`` and ``lists_theta`` (the theta in whose metric the final neighbour lists were built)."""

    def __init__(self, best, tries):
        self.theta, self.value, self.grad = best["theta"], best["value"], best["grad"]
        self.n_evaluations, self.n_refreshes, self.converged = best["n_evaluations"], best["n_refreshes"], best["converged"]
        self.tries = tries


class ExactFit(object):
    """What ``VecchiaGP.fit_exact`` returns: ``theta``, ``value`` (the estimated exact log-likelihood there, on the probes of the run), ``grad``
    (its gradient there), ``n_evaluations``, ``converged`` (L-BFGS-B ended by one of its own rules), ``message`` and ``loglik``, the
    ``ExactLogLik`` at ``theta``."""

    def __init__(self, theta, value, grad, n_evaluations, converged, message, loglik):
        self.theta, self.value, self.grad, self.n_evaluations = theta, value, grad, n_evaluations
        self.converged, self.message, self.loglik = converged, message, loglik


def _kernel_name(who, kernel):
    name = kernel if isinstance(kernel, str) else type(kernel).__name__
    if name == "ProductMat52":
        raise RuntimeError("%s: not available with the ProductMat52 kernel (not a function of one scaled distance)" % who)
    if name not in _KERNELS:
        raise ValueError("%s: kernel must be one of %s" % (who, ", ".join(sorted(_KERNELS))))
    return name


def _create_native(inputs, residuals, device):
    return _create_local_native(inputs, residuals, device)


class VecchiaGP(object):
    """``VecchiaGP(inputs, targets, kernel="SquaredExponential", n_neighbours=30, nugget="fit", order=None, rng=None, device=None)``

    ``inputs`` (N, D), ``targets`` (N,); THE MEAN IS ZERO (subtract one first).  ``kernel``: SquaredExponential, Matern52, UniformSqExp or
    UniformMat52, by name or instance.  ``nugget``: ``"fit"`` or a non-negative float held fixed.  ``order``: a permutation of 0 .. N-1, the
    Vecchia order (default: a random permutation from ``rng``, a seed or a ``numpy.random.Generator``; ``np.arange(N)`` keeps the caller's).
    The design is stored on the device in that order; every index this class returns is in the caller's numbering.

    Every argument is checked before the device is touched: ``ValueError`` for shapes, non-finite values, an ``order`` that is no permutation,
    ``n_neighbours`` outside 1 .. min(N - 1, 126) and a theta of the wrong length; ``RuntimeError`` for ``ProductMat52``, for
    ``nugget="adaptive"`` / ``"pivot"`` and for ``loglik`` before ``set_neighbours``.  The native handle is freed by ``close()``."""

    def __init__(self, inputs, targets, kernel="SquaredExponential", n_neighbours=30, nugget="fit", order=None, rng=None, device=None):
        who = "VecchiaGP"
        self._native = None
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        if inputs.ndim != 2 or inputs.shape[0] < 2 or inputs.shape[1] < 1:
            raise ValueError("%s: inputs must have shape (N, D) with at least two points" % who)
        N, D = inputs.shape
        if D > MAX_D:
            raise ValueError("%s: at most %d input dimensions" % (who, MAX_D))
        if N >= 2 ** 31 - 256:
            raise ValueError("%s: the design must have fewer than 2^31 - 256 points" % who)
        if not np.all(np.isfinite(inputs)):
            raise ValueError("%s: inputs must be finite" % who)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.shape != (N,):
            raise ValueError("%s: targets must have shape (N,) with N = %d" % (who, N))
        if not np.all(np.isfinite(targets)):
            raise ValueError("%s: targets must be finite" % who)
        name = _kernel_name(who, kernel)
        if isinstance(nugget, str):
            if nugget in ("adaptive", "pivot"):
                raise RuntimeError("%s: not available with nugget=\"%s\"" % (who, nugget))
            if nugget != "fit":
                raise ValueError("%s: nugget must be \"fit\" or a non-negative float" % who)
        else:
            nugget = float(nugget)
            if not (nugget >= 0. and np.isfinite(nugget)):
                raise ValueError("%s: nugget must be \"fit\" or a non-negative float" % who)
        k = int(n_neighbours)
        if k != n_neighbours or k < 1 or k > min(N - 1, MAX_NEIGHBOURS):
            raise ValueError("%s: n_neighbours must be between 1 and min(N - 1, %d) = %d" % (who, MAX_NEIGHBOURS, min(N - 1, MAX_NEIGHBOURS)))
        if order is None:
            order = np.random.default_rng(rng).permutation(N)
        else:
            order = np.asarray(order)
            if order.shape != (N,) or order.dtype.kind not in "iu" or not np.array_equal(np.sort(order), np.arange(N)):
                raise ValueError("%s: order must be a permutation of 0 .. N-1" % who)
        if device is not None and (int(device) != device or int(device) < 0):
            raise ValueError("%s: device must be a device ordinal or None" % who)
        self._order = order.astype(np.int64)
        self._kernel, (self._kt, self._uniform) = name, _KERNELS[name]
        self._N, self._D, self._k, self._nugget = N, D, k, nugget
        self._nc = 1 if self._uniform else D
        self._scales = self._nbr = self._fit = self._theta = None      # _theta: what predict uses, of the last fit or fit_exact
        self._range, self._tvar = inputs.max(axis=0) - inputs.min(axis=0), float(np.var(targets))
        self._native = _create_native(np.ascontiguousarray(inputs[self._order]), np.ascontiguousarray(targets[self._order][None, :]),
                                      None if device is None else int(device))

    n = property(lambda self: self._N)
    D = property(lambda self: self._D)
    n_neighbours = property(lambda self: self._k)
    n_params = property(lambda self: self._nc + 1 + (1 if self._nugget == "fit" else 0))
    kernel = property(lambda self: self._kernel)
    order = property(lambda self: self._order.copy())
    theta = property(lambda self: None if self._theta is None else self._theta.copy())

    def close(self):
        native, self._native = getattr(self, "_native", None), None
        if native is not None:
            native.close()

    def __del__(self):
        self.close()

    # ---- checks that need no device --------------------------------------------------------------------------------------------------
    def _hyper(self, who, theta):
        """(s (D,), sigma^2, nugget) of theta"""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.shape != (self.n_params,):
            raise ValueError("%s: theta must have %d entries" % (who, self.n_params))
        if not np.all(np.isfinite(theta)):
            raise ValueError("%s: theta must be finite" % who)
        with np.errstate(over="ignore"):
            s = np.sqrt(np.exp(theta[:self._nc]))
            sigma2 = float(np.exp(theta[self._nc]))
            nugget = float(np.exp(theta[self._nc + 1])) if self._nugget == "fit" else self._nugget
        s = np.full(self._D, s[0]) if self._uniform else np.ascontiguousarray(s)
        if not (np.all(np.isfinite(s)) and np.all(s > 0.) and np.isfinite(sigma2) and sigma2 > 0. and np.isfinite(nugget)):
            raise ValueError("%s: theta does not give positive finite scales and variances" % who)
        return s, sigma2, nugget

    def _open(self, who):
        if self._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        return self._native

    # ---- the neighbour lists -----------------------------------------------------------------------------------------------------------
    def set_neighbours(self, theta=None, scales=None):
        """Search, on the device, the ``n_neighbours`` nearest EARLIER points of every point in the metric s_d = sqrt(exp(theta_d)) (or the
        given ``scales`` (D,); default: all ones) and keep the lists there for every later ``loglik``."""
        who = "VecchiaGP.set_neighbours"
        if theta is not None and scales is not None:
            raise ValueError("%s: give theta or scales, not both" % who)
        if theta is not None:
            s = self._hyper(who, theta)[0]
        elif scales is not None:
            s = np.ascontiguousarray(scales, dtype=np.float64)
            if s.shape != (self._D,) or not np.all(np.isfinite(s)) or not np.all(s > 0.):
                raise ValueError("%s: scales must be %d positive finite numbers" % (who, self._D))
        else:
            s = np.ones(self._D)
        self._open(who).vecchia_neighbours(s, self._k, return_neighbours=False)
        self._scales, self._nbr = s.copy(), None

    @property
    def neighbours(self):
        """(N, k) int64 in the caller's numbering: row i holds the neighbours of point i, nearest first, -1 where it has fewer than k
        predecessors.  (Fetched on first use: the search runs once more with the lists copied out; it gives the same lists.)"""
        who = "VecchiaGP.neighbours"
        if self._scales is None:
            raise RuntimeError("%s: set_neighbours has not been called" % who)
        if self._nbr is None:
            pos = self._open(who).vecchia_neighbours(self._scales, self._k, return_neighbours=True)
            out = np.empty_like(pos)
            out[self._order] = np.where(pos >= 0, self._order[np.maximum(pos, 0)], -1)
            self._nbr = out
        return self._nbr.copy()

    # ---- the likelihood ----------------------------------------------------------------------------------------------------------------
    def loglik(self, theta, grad=False, return_terms=False, jitter=0.0, max_points=0):
        """The Vecchia log-likelihood at ``theta`` on the current neighbour lists; returns a ``VecchiaLogLik``.

        ``jitter`` >= 0 is added to the diagonal of every local matrix (a constant: it has no derivative).  A point whose matrix is not
        positive definite gets a NaN term and ``ok`` False and touches no other point; ``value`` is then ``-inf`` and ``grad`` NaN.
        ``max_points`` caps the points per device launch and changes no bit of the result."""
        who = "VecchiaGP.loglik"
        s, sigma2, nugget = self._hyper(who, theta)
        jitter = float(jitter)
        if not (jitter >= 0. and np.isfinite(jitter)):
            raise ValueError("%s: jitter must be a finite number that is not negative" % who)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if self._scales is None:
            raise RuntimeError("%s: set_neighbours has not been called" % who)
        value, g, terms, ok = self._open(who).vecchia_loglik(0, self._kt, s, sigma2, nugget, jitter, self._k, grad=bool(grad),
                                                             return_terms=bool(return_terms), max_points=int(max_points))
        failed = not ok.all()
        out_g = None
        if grad:
            corr = g[:self._D]
            if self._uniform:
                tot = 0.
                for x in corr:                   # ascending in d
                    tot = tot + x
                corr = np.array([tot])
            out_g = np.concatenate([corr, g[self._D:self._D + 1], g[self._D + 1:] if self._nugget == "fit" else []])
            if failed:
                out_g = np.full(self.n_params, np.nan)
        ok_c = np.empty_like(ok)
        ok_c[self._order] = ok
        terms_c = None
        if return_terms:
            terms_c = np.empty_like(terms)
            terms_c[self._order] = terms
        return VecchiaLogLik(-np.inf if failed else value, out_g, terms_c, ok_c)

    # ---- the fit ------------------------------------------------------------------------------------------------------------------------
    def default_theta(self):
        """the start of ``fit`` without ``theta0``: correlation lengths of 0.3 sqrt(D) times the range of every input, sigma^2 = the variance of
        the targets, nugget = 10^-3 of it"""
        corr = -2. * np.log(0.3 * np.sqrt(self._D) * np.maximum(self._range, 1e-12))
        corr = np.array([corr.mean()]) if self._uniform else corr
        lv = np.log(max(self._tvar, 1e-300))
        return np.concatenate([corr, [lv], [lv + np.log(1e-3)] if self._nugget == "fit" else []])

    def fit(self, theta0=None, n_tries=1, refresh=2, rng=None, **lbfgs_options):
        """Maximise the Vecchia likelihood: ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)`` on ``-loglik``; no priors.

        Every try builds the neighbour lists in the metric of its start; after each convergence they are rebuilt in the metric of the
        current estimate and the optimisation is resumed from it, ``refresh`` times ("scaled Vecchia").  ``theta0`` (P,) or None (``default_theta()``: a start
        from the ranges of the data); tries after the first start
        from ``theta0`` plus standard normal noise from ``rng``.  ``lbfgs_options`` go to the optimiser's ``options``; the defaults are
        ``gtol = 1e-5 N`` (the projected-gradient rule on the MEAN log-likelihood at SciPy's own 1e-5), ``ftol = 1e-13``, ``maxiter = 200``.
        A non-finite evaluation is handed to the optimiser as a large finite value with a zero gradient.  Returns a ``VecchiaFit`` (also kept:
        ``predict`` uses its theta)."""
        from scipy.optimize import minimize
        who = "VecchiaGP.fit"
        if int(n_tries) != n_tries or int(n_tries) < 1:
            raise ValueError("%s: n_tries must be at least 1" % who)
        if int(refresh) != refresh or int(refresh) < 0:
            raise ValueError("%s: refresh must not be negative" % who)
        if theta0 is not None:
            theta0 = np.array(theta0, dtype=np.float64)
            self._hyper(who, theta0)
        self._open(who)
        if theta0 is None:
            theta0 = self.default_theta()
        options = dict(gtol=1e-5 * self._N, ftol=1e-13, maxiter=200)
        options.update(lbfgs_options)
        gen = np.random.default_rng(rng)
        count = [0]

        def objective(th):
            count[0] += 1
            try:
                ll = self.loglik(th, grad=True)
            except ValueError:                   # theta outside what exp() holds
                return _FAILED, np.zeros(self.n_params)
            if not (np.isfinite(ll.value) and np.all(np.isfinite(ll.grad))):
                return _FAILED, np.zeros(self.n_params)
            return -ll.value, -ll.grad

        tries = []
        for i in range(int(n_tries)):
            start = theta0 if i == 0 else theta0 + gen.standard_normal(self.n_params)
            count[0] = 0
            self.set_neighbours(theta=start)
            start_value = self.loglik(start).value
            th, converged, done, lists = start, True, 0, start
            for r in range(int(refresh) + 1):
                if r > 0:
                    self.set_neighbours(theta=th)
                    done, lists = done + 1, th
                res = minimize(objective, th, method="L-BFGS-B", jac=True, options=options)
                th, converged = np.array(res.x, dtype=np.float64), converged and bool(res.success)
            tries.append(dict(theta0=start.copy(), start_value=start_value, theta=th, value=-float(res.fun), grad=-np.array(res.jac, dtype=np.float64),
                              n_evaluations=count[0], n_refreshes=done, converged=converged, message=str(res.message),
                              lists_theta=np.array(lists, dtype=np.float64)))
        best = max(tries, key=lambda t: t["value"] if np.isfinite(t["value"]) and t["value"] > -_FAILED else -np.inf)
        if best is not tries[-1]:
            self.set_neighbours(theta=best["lists_theta"])     # the lists on the device are those the kept value was computed on
        self._fit = VecchiaFit(best, tries)
        self._theta = self._fit.theta
        return self._fit

    # ---- prediction ---------------------------------------------------------------------------------------------------------------------
    def predict(self, testing, n_neighbours=None, theta=None, **kw):
        """``LocalGP.predict`` at the fitted theta (or ``theta``) on the same native handle -- the design is not uploaded again.
        ``n_neighbours``: the neighbours of a QUERY, 1 .. min(N, 126) (default: the Vecchia k); ``kw`` as ``LocalGP.predict`` takes them.
        Returns a ``LocalPrediction`` whose neighbour indices are in the caller's numbering."""
        who = "VecchiaGP.predict"
        if theta is None:
            if self._theta is None:
                raise RuntimeError("%s: fit has not been called and no theta was given" % who)
            theta = self._theta
        s, sigma2, nugget = self._hyper(who, theta)
        k = self._k if n_neighbours is None else n_neighbours
        view = _LocalGP._on_handle(self._open(who), [(self._kt, s, sigma2, nugget, None, np.zeros(0))], self._D, self._N, k)
        p = view.predict(testing, **kw)
        if p.neighbours is not None:
            p.neighbours = self._order[p.neighbours]
        return p

    def predict_exact(self, testing, theta=None, **kw):
        """``IterativeGP.predict`` at the fitted theta (or ``theta``) on the same native handle: the exact posterior of all N points by
        preconditioned conjugate gradients, where ``predict`` answers from the neighbours of a query.  ``precond_rank``, ``rtol`` and
        ``max_iter`` of ``kw`` go to ``IterativeGP``, the rest to its ``predict`` (``unc="bound"`` among them: the conservative variance of
        ``IterativeGP.variance_bound`` in place of one solve per query; ``deriv=True``: the derivative of the mean with respect to the
        inputs, ``IterativePrediction.deriv`` (m, D)).  Returns an ``IterativePrediction``; the nugget must be positive.  ``predict``
        is unchanged."""
        options = {k: kw.pop(k) for k in ("precond_rank", "rtol", "max_iter") if k in kw}
        return self._exact_view("VecchiaGP.predict_exact", theta, options).predict(testing, **kw)

    def sample_paths(self, n_draws=1, theta=None, **kw):
        """``IterativeGP.sample_paths`` at the fitted theta (or ``theta``) on the same native handle: ``n_draws`` functions from the exact
        posterior of all N points, each to be evaluated at any query set.  ``precond_rank``, ``rtol`` and ``max_iter`` of ``kw`` go to
        ``IterativeGP``, the rest to its ``sample_paths``.  Returns a ``PosteriorPaths``; its ``update`` -- and the columns of a
        ``noise_normals`` given -- are in the Vecchia order of the handle (``order``), what it evaluates to has no such index."""
        options = {k: kw.pop(k) for k in ("precond_rank", "rtol", "max_iter") if k in kw}
        return self._exact_view("VecchiaGP.sample_paths", theta, options).sample_paths(n_draws, **kw)

    def exact_view(self, theta=None, **options):
        """An ``IterativeGP`` on this object's native handle at the fitted theta (or ``theta``), for ``matvec`` / ``solve`` / ``weights``;
        ``options``: ``precond_rank``, ``rtol``, ``max_iter``.  THE HANDLE HOLDS THE DESIGN IN THE VECCHIA ORDER: rows of what the view takes
        and returns are in that order (``order``); ``weights_in_callers_order`` undoes it.  ``predict`` of the view has no such index."""
        return self._exact_view("VecchiaGP.exact_view", theta, options)

    def _exact_view(self, who, theta, options):
        if theta is None:
            if self._theta is None:
                raise RuntimeError("%s: fit has not been called and no theta was given" % who)
            theta = self._theta
        s, sigma2, nugget = self._hyper(who, theta)
        return _IterativeGP._on_handle(self._open(who), [(self._kt, s, sigma2, nugget, None, np.zeros(0))], self._D, self._N,
                                       layout=[(self._uniform, self._nugget == "fit")], **options)

    # ---- the exact likelihood -----------------------------------------------------------------------------------------------------------
    def loglik_exact(self, theta, grad=False, n_probes=15, seed=0, probes=None, precond_rank=256, rtol=1e-8, max_iter=1000, probe_terms=False):
        """The EXACT log-likelihood of the whole design at ``theta`` (laid out as for ``loglik``) and, with ``grad=True``, its gradient, by
        ``IterativeGP.log_likelihood`` on this object's native handle: one preconditioned CG solve of [y | probes] and stochastic Lanczos
        quadrature.  Returns an ``ExactLogLik``; the nugget must be positive.  ``probes=(g1, g2)``: the caller's normals, g2's rows in the
        Vecchia order of the handle (``order``).  Needs no neighbour lists."""
        who = "VecchiaGP.loglik_exact"
        s, sigma2, nugget = self._hyper(who, theta)
        if not nugget > 0.:
            raise ValueError("%s: the nugget must be positive (the preconditioner divides by it)" % who)
        p, rtol, max_iter = _check_options(who, self._N, precond_rank, rtol, max_iter)
        T, seed, g2, g1 = _check_probes(who, n_probes, seed, probes, self._N)
        return _exact_loglik(who, self._open(who), 0, (self._kt, s, sigma2, nugget), (self._uniform, self._nugget == "fit"), self._D, self._N, p,
                             rtol, max_iter, bool(grad), T, seed, g1, g2, bool(probe_terms) and bool(grad))

    def fit_exact(self, theta0=None, n_probes=15, seed=0, precond_rank=256, rtol=1e-8, max_iter=1000, **lbfgs_options):
        """Maximise the exact log-likelihood: ``scipy.optimize.minimize(method="L-BFGS-B", jac=True)`` on ``-loglik_exact``; no priors.

        The normals of the probes are those of ``seed`` for the whole run -- the probes z = L g1 + sqrt(nugget) g2 follow theta through L
        and the nugget -- so the objective is a deterministic function of theta.  ``theta0`` (P,) or None: the Vecchia fit (``fit()`` is run
        when it has not been).  ``lbfgs_options`` go to the optimiser's ``options`` (defaults as ``fit``).  An evaluation that is not finite
        or whose solve did not converge is handed to the optimiser as a large finite value with a zero gradient.  Returns an ``ExactFit``;
        the theta is also kept (``theta``; ``predict`` / ``predict_exact`` use it), the record of the Vecchia fit is left as it is."""
        from scipy.optimize import minimize
        who = "VecchiaGP.fit_exact"
        if theta0 is not None:
            theta0 = np.array(theta0, dtype=np.float64)
            if not self._hyper(who, theta0)[2] > 0.:
                raise ValueError("%s: the nugget must be positive (the preconditioner divides by it)" % who)
        elif not (self._nugget == "fit" or self._nugget > 0.):
            raise ValueError("%s: the nugget must be positive (the preconditioner divides by it)" % who)
        _check_options(who, self._N, precond_rank, rtol, max_iter)
        _check_probes(who, n_probes, seed, None, self._N)
        self._open(who)
        if theta0 is None:
            theta0 = (self._fit if self._fit is not None else self.fit()).theta
        options = dict(gtol=1e-5 * self._N, ftol=1e-13, maxiter=200)
        options.update(lbfgs_options)
        kw = dict(n_probes=n_probes, seed=seed, precond_rank=precond_rank, rtol=rtol, max_iter=max_iter)
        count = [0]

        def objective(th):
            count[0] += 1
            try:
                ll = self.loglik_exact(th, grad=True, **kw)
            except ValueError:                   # theta outside what exp() holds
                return _FAILED, np.zeros(self.n_params)
            if not (ll.ok and np.isfinite(ll.value) and np.all(np.isfinite(ll.grad))):
                return _FAILED, np.zeros(self.n_params)
            return -ll.value, -ll.grad

        res = minimize(objective, theta0, method="L-BFGS-B", jac=True, options=options)
        theta = np.array(res.x, dtype=np.float64)
        final = self.loglik_exact(theta, grad=True, **kw)
        self._theta = theta
        return ExactFit(theta, final.value, final.grad, count[0], bool(res.success), str(res.message), final)

    def weights_in_callers_order(self, view):
        """alpha of ``view`` (an ``exact_view``) with entry i belonging to design point i of the caller"""
        out = np.empty(self._N)
        out[self._order] = view.weights()
        return out
