"""NumPy restatement of the dense zero-mean GP (log-likelihood, its gradient, prediction with the input derivative of the mean and the full
covariance), written from the definitions and independent of the package's own code, in float64 and in np.longdouble, for the
squared-exponential, the Matern-5/2 and the product-of-Matern-5/2 kernels.  It builds on local_restate's cholesky and forward and on
vecchia_restate's backward.

theta = [correlation raws (D) | log sigma^2 | log nugget if fitted].  The scales s_d = sqrt(exp(theta_d)) are taken in float64, as the host
hands them to the device; the scaled coordinates u = x s, their differences and everything behind them are in the dtype asked for.  With
q_d = (u_id - u_jd)^2 and r2 = sum_d q_d:
    SquaredExponential  k = exp(-r2 / 2)                                   dk/dq_d = -k / 2
    Matern52            k = (1 + a + a^2 / 3) exp(-a), a = sqrt(5 r2)      dk/dq_d = -(5 / 6) (1 + a) exp(-a)
    ProductMat52        k = prod_d m(q_d), m the Matern-5/2 of one q       dk/dq_d = m'(q_d) prod_(e != d) m(q_e)
    dk / dtheta_d = (dk/dq_d) q_d                    dk(x*, x_j) / dx*_d = (dk/dq_d) 2 (u*_d - u_jd) s_d
A = sigma^2 k + eta I = L L^T, alpha = A^-1 y:
    log-likelihood  -sum log L_ii - y^T alpha / 2 - n log(2 pi) / 2,      d / dp = alpha^T A_p alpha / 2 - tr(A^-1 A_p) / 2
    mean  k*^T alpha,   variance  sigma^2 + eta - |L^-1 k*|^2 (eta only with include_nugget),   covariance  K** + eta I - (L^-1 K*)^T (L^-1 K*)
The package's log-posterior under weak priors is MINUS the log-likelihood."""
import numpy as np

import local_restate as lr
from vecchia_restate import backward

KERNELS = ("SquaredExponential", "Matern52", "ProductMat52")


def scales(theta, D):
    return np.sqrt(np.exp(np.asarray(theta, dtype=np.float64)[:D]))


def _mat52(q, dt):
    a = np.sqrt(dt(5) * q)
    e = np.exp(-a)
    return (dt(1) + a + a * a / dt(3)) * e, -(dt(5) / dt(6)) * (dt(1) + a) * e


def kernel(U1, U2, kind, dtype, deriv=False):
    """(k (n1, n2), dk/dq_d (D, n1, n2) or None, the differences u1_id - u2_jd (D, n1, n2)) of scaled points"""
    dt = np.dtype(dtype).type
    diff = np.stack([U1[:, d][:, None] - U2[:, d][None, :] for d in range(U1.shape[1])])
    q = diff * diff
    D = q.shape[0]
    if kind == "ProductMat52":
        m, dm = _mat52(q, dt)
        k = np.ones(q.shape[1:], dtype=dtype)
        for d in range(D):
            k = k * m[d]
        dk = None
        if deriv:
            dk = np.empty_like(q)
            for d in range(D):
                f = dm[d]
                for e in range(D):
                    if e != d:
                        f = f * m[e]
                dk[d] = f
        return k, dk, diff
    r2 = np.zeros(q.shape[1:], dtype=dtype)
    for d in range(D):
        r2 = r2 + q[d]
    if kind == "Matern52":
        k, d1 = _mat52(r2, dt)
    else:
        assert kind == "SquaredExponential", kind
        k = np.exp(-r2 / dt(2))
        d1 = -k / dt(2)
    return k, (np.broadcast_to(d1, q.shape) if deriv else None), diff


def _log_2pi(dt):
    return np.log(dt(8) * np.arctan(dt(1)))


class Dense(object):
    """the factorised model at one theta; raises np.linalg.LinAlgError where the Cholesky factorisation refuses"""

    def __init__(self, X, y, theta, kind, nugget, dtype=np.float64):
        dt = self.dt = np.dtype(dtype).type
        self.dtype, self.kind = dtype, kind
        theta = np.asarray(theta, dtype=np.float64)
        self.n, self.D = np.shape(X)
        self.fit = isinstance(nugget, str)
        assert theta.shape == (self.D + 1 + (1 if self.fit else 0),)
        self.s = np.asarray(scales(theta, self.D), dtype=dtype)
        self.sigma2 = np.exp(dt(theta[self.D]))
        self.eta = np.exp(dt(theta[self.D + 1])) if self.fit else dt(nugget)
        self.U = np.asarray(X, dtype=dtype) * self.s
        self.y = np.asarray(y, dtype=dtype)
        k, self.dk, diff = kernel(self.U, self.U, kind, dtype, deriv=True)
        self.q = diff * diff
        self.K = self.sigma2 * k
        self.A = self.K + self.eta * np.eye(self.n, dtype=dtype)
        self.L = lr.cholesky(self.A)
        self.z = lr.forward(self.L, self.y[:, None])[:, 0]
        self.alpha = backward(self.L, self.z[:, None])[:, 0]

    def loglik(self):
        dt = self.dt
        return -np.sum(np.log(np.diag(self.L))) - self.z @ self.z / dt(2) - dt(self.n) * _log_2pi(dt) / dt(2)

    def grad(self):
        dt, a = self.dt, self.alpha
        eye = np.eye(self.n, dtype=self.dtype)
        Ainv = backward(self.L, lr.forward(self.L, eye))

        def entry(Ap):
            return a @ Ap @ a / dt(2) - np.sum(Ainv * Ap) / dt(2)
        g = [entry(self.sigma2 * self.dk[d] * self.q[d]) for d in range(self.D)] + [entry(self.K)]
        if self.fit:
            g.append(entry(self.eta * eye))
        return np.array(g, dtype=self.dtype)

    def predict(self, Xs, include_nugget=True):
        """dict(mean (m,), var (m,), deriv (m, D), fullcov (m, m))"""
        dt = self.dt
        Us = np.asarray(Xs, dtype=self.dtype) * self.s
        k, dk, diff = kernel(Us, self.U, self.kind, self.dtype, deriv=True)                 # (m, n)
        Ks = self.sigma2 * k
        V = lr.forward(self.L, Ks.T.copy())                                                # (n, m)
        nug = self.eta if include_nugget else dt(0)
        var = self.sigma2 + nug - np.sum(V * V, axis=0)
        kss = kernel(Us, Us, self.kind, self.dtype)[0]
        cov = self.sigma2 * kss + nug * np.eye(Us.shape[0], dtype=self.dtype) - V.T @ V
        deriv = np.stack([(self.sigma2 * dk[d] * dt(2) * diff[d] * self.s[d]) @ self.alpha for d in range(self.D)], axis=1)
        return dict(mean=Ks @ self.alpha, var=np.where(var > 0, var, dt(0)), deriv=deriv, fullcov=cov)
