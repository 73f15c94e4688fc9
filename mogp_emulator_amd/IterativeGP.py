"""
Exact GP prediction for designs far beyond what one dense factorisation holds: conjugate gradients on the covariance matrix of the WHOLE
design, matrix-free and preconditioned (Gardner et al. 2018; Wang et al. 2019).

    s_d = sqrt(exp(theta_d))                              (one shared value for the uniform kernels)
    A = sigma^2 k(r2(x_i s, x_j s)) + nugget I            N x N, never stored: its entries are generated as they are multiplied
    alpha = A^-1 (y - m(X))                               preconditioned CG, P = L L^T + nugget I, L a rank-p pivoted Cholesky factor
    mean = m(q) + k*^T alpha,    unc = max(sigma^2 - k*^T A^-1 k* + nugget, 0)

``LocalGP`` answers from at most 126 neighbours of a query; this class gives what the dense ``predict`` would give at the same
hyperparameters -- the posterior of all N points -- at the price of one product with A (N^2 generated entries) per iteration.  The
hyperparameters come from a fitted ``GaussianProcessGPU`` / ``MultiOutputGP_GPU`` (typically fitted on a subsample) or from
``VecchiaGP.fit`` (``VecchiaGP.predict_exact``).  The design and the mean-subtracted targets go up once (``csrc/kernels_iter.hip``,
``csrc/engine_iter.hip``; the native handle is ``LocalGP``'s).

Every column of a solve is its own problem: it stops as soon as ITS recurrence residual satisfies |r| <= rtol |b| and is never touched again,
so a result depends neither on the columns it shares a block with nor on ``max_points``; nothing uses atomics, a repeated call returns the
same bits.  What is reported as ``residual`` is |b - A x| / |b| recomputed with one further product, as it is: a column that did not
converge within ``max_iter`` is not an error, it comes back with ``converged`` False and its honest residual.

Not covered: estimating theta or the log-determinant iteratively, cheap approximate variances (every variance is a solve), the symmetry of A
in the product, several devices per handle, ``ProductMat52``, ``analytic_mean=True``, ``nugget="pivot"``.
"""
import numpy as np

from .LocalGP import MAX_D, _create_native, _emulator_type, _fit_state, _hyperparameters, _mean_at, _points

MAX_RANK = 1024


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
    * ``var_converged``, ``var_residual``           per query, of the solve behind its variance; None with ``unc=False``"""

    def __init__(self, mean, unc, converged, residual, iterations, var_converged, var_residual):
        self.mean, self.unc, self.converged, self.residual, self.iterations = mean, unc, converged, residual, iterations
        self.var_converged, self.var_residual = var_converged, var_residual


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
        _check_nuggets(who, self._hyper)
        self._single, self._D, self._N, self._E = single, D, N, E
        resid = np.stack([targets[e] - _mean_at(h[4], h[5], inputs) for e, h in enumerate(self._hyper)])
        self._native = _create_native(inputs, np.ascontiguousarray(resid), None if device is None else int(device))

    @classmethod
    def _on_handle(cls, native, hyper, D, N, precond_rank=256, rtol=1e-8, max_iter=1000):
        """Internal: a single-output view on a native handle that somebody else owns (``VecchiaGP.predict_exact``), at the hyperparameters
        ``hyper`` = [(kernel 0 / 1, s (D,), sigma^2, nugget, mean function or None, its parameters)] in place of a fitted ``gp``.
        ``close()`` of the view leaves the handle open."""
        who = "IterativeGP"
        self = cls.__new__(cls)
        self._p, self._rtol, self._max_iter = _check_options(who, int(N), precond_rank, rtol, max_iter)
        _check_nuggets(who, hyper)
        self._single, self._D, self._N, self._E = True, int(D), int(N), 1
        self._hyper, self._native, self._borrowed = list(hyper), native, True
        return self

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

    # ---- prediction ----------------------------------------------------------------------------------------------------------------------
    def predict(self, testing, unc=False, include_nugget=True, max_points=0):
        """Predict at ``testing`` (m, D) from the whole design; returns an ``IterativePrediction``.

        ``unc=True`` solves one system per query (in blocks of 32): exact, and as expensive as that sounds.  ``include_nugget``: add the
        nugget to ``unc`` as ``predict`` of the emulator does.  ``max_points`` caps the queries per device pass (0: sized by the free device
        memory) and changes no bit of the result.  Emulator e of a ``MultiOutputGP_GPU`` uses its own hyperparameters and its own
        preconditioner; the emulators run one after another on the same handle, and row e equals the single-emulator call bit for bit."""
        who = "IterativeGP.predict"
        testing = _points("testing", who, testing, self._D)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        if self._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        rows = []
        for e, (kt, s, sigma2, nugget, meanfunc, mparams) in enumerate(self._hyper):
            mean, var, (it, cv, res), vstats, _ = self._native.predict_exact(e, kt, s, sigma2, nugget, self._p, self._rtol, self._max_iter,
                                                                             include_nugget, testing, unc=bool(unc), max_points=int(max_points))
            mean += _mean_at(meanfunc, mparams, testing)
            rows.append((mean, var, cv, res, it, vstats[1] if unc else None, vstats[2] if unc else None))
        if self._single:
            return IterativePrediction(*rows[0])
        cols = list(zip(*rows))
        return IterativePrediction(np.stack(cols[0]), np.stack(cols[1]) if unc else None, np.array(cols[2]), np.array(cols[3]), np.array(cols[4]),
                                   np.stack(cols[5]) if unc else None, np.stack(cols[6]) if unc else None)
