"""
Hessian of the negative log-posterior at a hyperparameter vector, computed on the device (``csrc/kernels_hess.hip``), and the Laplace
approximation of the hyperparameter posterior around a MAP fit.

With theta = [corr_raw | log sigma^2 | log nugget (fitted nugget only)], Q = sigma^2 C + nugget I, alpha = Q^-1 t and F the negative
log-posterior,

    F_pq = alpha^T Q_p Q^-1 Q_q alpha - 1/2 alpha^T Q_pq alpha - 1/2 tr(Q^-1 Q_p Q^-1 Q_q) + 1/2 tr(Q^-1 Q_pq) - delta_pq d2 log p / d theta_p^2

where Q_p, Q_pq are the first and second derivatives of Q.  An adaptive or fixed nugget is a constant, as in the gradient.  At a MAP
point theta_hat the posterior is approximately N(theta_hat, H^-1): the square roots of the diagonal of H^-1 say how well the data
determine each hyperparameter, and an eigenvalue of H that is not positive says the optimiser stopped at a saddle or on a ridge.

``GaussianProcessGPU.logpost_hessian`` keeps raising ``GPUUnavailableError`` as the reference interface does; the feature lives here.
Not covered (``RuntimeError``): ``nugget="pivot"``, ``analytic_mean=True``, mean functions with parameters in theta, ``ProductMat52``.
"""
import numpy as np


def _theta_of(emulator):
    th = emulator.get_theta()
    return np.concatenate([th.get_mean(), th.get_data()]) if th.data_has_been_set() else None


class HessianStack(np.ndarray):
    """(n_emulators, P, P) array of Hessians with ``fitted``: the indices of the emulators that were evaluated (the blocks of
    the others are NaN), and ``ok``: per emulator, whether its Hessian was computed."""

    def __new__(cls, hess, fitted, ok):
        obj = np.asarray(hess).view(cls)
        obj.fitted = list(fitted)
        obj.ok = np.asarray(ok, dtype=bool)
        return obj

    def __array_finalize__(self, obj):
        self.fitted = getattr(obj, "fitted", [])
        self.ok = getattr(obj, "ok", None)


def logpost_hessian(gp, theta=None):
    """Hessian of the negative log-posterior of ``gp`` at ``theta`` (default: the fitted theta).

    ``GaussianProcessGPU``: ``theta`` (P,) -> (P, P).  ``MultiOutputGP_GPU``: ``theta`` (n_emulators, P) or None -> (n_emulators, P, P)
    from one batched device call; with ``theta=None`` the emulators that are not fit give NaN blocks and the result's ``fitted``
    attribute lists the ones that are.  Both triangles are filled and exactly equal; two calls return the same bits; the cached state
    of a fitted emulator is not changed by the call."""
    from .GaussianProcessGPU import GaussianProcessGPU
    from .MultiOutputGP_GPU import MultiOutputGP_GPU
    if isinstance(gp, GaussianProcessGPU):
        if theta is None:
            theta = _theta_of(gp._densegp_gpu)
            if theta is None:
                raise ValueError("hyperparameters have not been fit for this Gaussian Process")
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (gp.n_params,):
            raise ValueError("theta must have shape (n_params,)")
        return gp._densegp_gpu.logpost_hessian(theta)
    if isinstance(gp, MultiOutputGP_GPU):
        ne = gp.n_emulators
        width = max(gp.n_params)
        if theta is None:
            fitted = gp.get_indices_fit()
            rows = np.full((ne, width), np.nan)
            for i in fitted:
                th = _theta_of(gp._mogp_gpu.emulator(i))
                rows[i, :th.size] = th
        else:
            rows = np.ascontiguousarray(theta, dtype=np.float64)
            if rows.shape != (ne, width):
                raise ValueError("theta must have shape (n_emulators, n_params)")
            fitted = [i for i in range(ne) if not np.isnan(rows[i, 0])]
        hess, ok = gp._mogp_gpu.hessian(rows)
        return HessianStack(hess, fitted, ok)
    raise TypeError("logpost_hessian needs a GaussianProcessGPU or a MultiOutputGP_GPU")


class LaplaceResult(object):
    """Gaussian approximation N(theta, hessian^-1) of the hyperparameter posterior.

    ``is_minimum``: the smallest eigenvalue of the Hessian is positive.  Then ``covariance`` is the inverse (through a Cholesky factor
    on the host) and ``stderr`` the square roots of its diagonal; otherwise both are NaN -- no jitter is added and nothing is raised,
    because a saddle is information."""

    def __init__(self, theta, hessian):
        self.theta = np.array(theta, dtype=np.float64).reshape(-1)
        self.hessian = np.array(hessian, dtype=np.float64)
        P = self.theta.size
        if self.hessian.shape != (P, P):
            raise ValueError("hessian must have shape (len(theta), len(theta))")
        self.eigenvalues = np.full(P, np.nan)
        self.covariance = np.full((P, P), np.nan)
        self.stderr = np.full(P, np.nan)
        self._chol_cov = None
        self._chol_hess = None
        self.is_minimum = False
        if not np.all(np.isfinite(self.hessian)):
            return
        self.eigenvalues = np.linalg.eigvalsh(0.5 * (self.hessian + self.hessian.T))
        self.is_minimum = bool(self.eigenvalues[0] > 0.)
        if not self.is_minimum:
            return
        try:
            L = np.linalg.cholesky(self.hessian)
        except np.linalg.LinAlgError:           # positive in exact arithmetic only
            self.is_minimum = False
            return
        Linv = np.linalg.solve(L, np.eye(P))
        self.covariance = Linv.T @ Linv
        self.stderr = np.sqrt(np.diag(self.covariance))
        self._chol_cov = Linv.T                 # covariance = Linv^T Linv
        self._chol_hess = L

    def sample(self, n, rng=None):
        """``n`` draws theta ~ N(theta_hat, H^-1), shape (n, P); ``rng``: a ``numpy.random.Generator``, a seed or None"""
        if not self.is_minimum:
            raise ValueError("the Hessian is not positive definite: there is no Gaussian to sample from")
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        z = rng.standard_normal((int(n), self.theta.size))
        return self.theta + z @ self._chol_cov.T

    def logpdf(self, thetas):
        """log N(theta; theta_hat, H^-1) of every row of ``thetas`` (S, P) -- or of one theta (P,) -- with its constant:
        -P/2 log 2 pi + 1/2 log|H| - 1/2 (theta - theta_hat)^T H (theta - theta_hat), through the Cholesky factor of H"""
        if not self.is_minimum:
            raise ValueError("the Hessian is not positive definite: there is no Gaussian density")
        th = np.asarray(thetas, dtype=np.float64)
        P = self.theta.size
        if th.shape[-1:] != (P,) or th.ndim > 2:
            raise ValueError("thetas must have shape (S, %d) or (%d,)" % (P, P))
        y = (th - self.theta) @ self._chol_hess                           # rows (theta - theta_hat)^T L,  H = L L^T
        return -0.5 * P * np.log(2. * np.pi) + np.sum(np.log(np.diag(self._chol_hess))) - 0.5 * np.sum(y * y, axis=-1)

    def __repr__(self):
        return "LaplaceResult(is_minimum=%s, theta=%s, stderr=%s)" % (self.is_minimum, self.theta, self.stderr)


def laplace_approximation(gp):
    """``LaplaceResult`` of a fitted ``GaussianProcessGPU``, or a list with one entry per emulator of a ``MultiOutputGP_GPU`` (None
    for the emulators that are not fit); the Hessians of a multi-output model come from one batched device call."""
    from .GaussianProcessGPU import GaussianProcessGPU
    if isinstance(gp, GaussianProcessGPU):
        theta = _theta_of(gp._densegp_gpu)
        if theta is None:
            raise ValueError("hyperparameters have not been fit for this Gaussian Process")
        return LaplaceResult(theta, logpost_hessian(gp, theta))
    hess = logpost_hessian(gp)
    out = [None] * gp.n_emulators
    for i in hess.fitted:
        th = _theta_of(gp._mogp_gpu.emulator(i))
        out[i] = LaplaceResult(th, np.asarray(hess[i])[:th.size, :th.size])
    return out
