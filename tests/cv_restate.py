"""NumPy restatement of cross-validation at fixed hyperparameters ("Cross-validation"), independent of the product: no
import from mogp_emulator_amd.  Two forms of the same quantities, each in the dtype asked for (float64 or np.longdouble), with the
kernels and the plain Cholesky of marginal_restate.py:

fast   from the full matrix: Q = sigma^2 k + eta I, alpha = Q^-1 r, r = t - mean(X); for a fold F with S = (Q^-1)_FF = L_S L_S^T and
       y = L_S^-1 alpha_F:   e_F = L_S^-T y,   var_i = sum_k (L_S^-1)[k][i]^2,   mahalanobis = y^T y,
       log_score = -1/2 y^T y + sum log diag L_S - |F|/2 log 2 pi,   mean_i = t_i - e_i
brute  a refit per fold at the same theta: with R the other points, mu_F = mean + Q_FR Q_RR^-1 r_R, Sigma_F = Q_FF - Q_FR Q_RR^-1 Q_RF
       (the nugget included: the covariance of the observations), e_F = t_F - mu_F, mahalanobis = e^T Sigma^-1 e,
       log_score = -1/2 e^T Sigma^-1 e - 1/2 log|Sigma| - |F|/2 log 2 pi

theta, kernel and mean as in marginal_restate.py.  Both return a dict: mean, var (n,) with the nugget, mahalanobis, log_score (k,), eta.
"""
import numpy as np

from marginal_restate import PER_DIM, UNIFORM, _kernel, _mean_at, cholesky, lower_inverse, n_mean_params


def build(X, t, theta, kernel="SquaredExponential", mean="zero", nugget_fit=False, nugget=None, dtype=np.float64):
    """(Q, r, eta): the factored matrix, the residual targets and the nugget on the diagonal"""
    dt = np.dtype(dtype).type
    X = np.asarray(X, dtype=dtype)
    t = np.asarray(t, dtype=dtype)
    theta = np.asarray(theta, dtype=dtype)
    n, D = X.shape
    uniform = kernel in UNIFORM
    base = UNIFORM[kernel] if uniform else PER_DIM[kernel]
    nc = 1 if uniform else D
    nm = n_mean_params(mean)
    assert theta.shape == (nm + nc + 1 + (1 if nugget_fit else 0),)
    data = theta[nm:]
    scale = np.exp(data[:nc]) if not uniform else np.full(D, np.exp(data[0]), dtype=dtype)
    sig2 = np.exp(data[nc])
    eta = np.exp(data[nc + 1]) if nugget_fit else dt(nugget)
    r2 = (((X[:, None, :] - X[None, :, :]) ** 2) * scale).sum(-1)
    Q = sig2 * _kernel(base, r2, dt) + eta * np.eye(n, dtype=dtype)
    return Q, t - _mean_at(mean, theta, n, dt), eta


def _log_2pi(dt):
    return np.log(dt(8) * np.arctan(dt(1)))


def _folds(labels, k):
    labels = np.asarray(labels)
    assert labels.min() >= 0 and labels.max() < k
    return [np.flatnonzero(labels == f) for f in range(k)]


def fast(X, t, theta, labels, k, kernel="SquaredExponential", mean="zero", nugget_fit=False, nugget=None, dtype=np.float64):
    dt = np.dtype(dtype).type
    Q, r, eta = build(X, t, theta, kernel, mean, nugget_fit, nugget, dtype)
    n = Q.shape[0]
    Li = lower_inverse(cholesky(Q))
    Qinv = Li.T @ Li
    alpha = Li.T @ (Li @ r)
    tt = np.asarray(t, dtype=dtype)
    out = {"mean": np.zeros(n, dtype=dtype), "var": np.zeros(n, dtype=dtype), "mahalanobis": np.zeros(k, dtype=dtype),
           "log_score": np.zeros(k, dtype=dtype), "eta": eta}
    for f, F in enumerate(_folds(labels, k)):
        Ls = cholesky(Qinv[np.ix_(F, F)])
        Lsi = lower_inverse(Ls)
        y = Lsi @ alpha[F]
        e = Lsi.T @ y
        out["mean"][F] = tt[F] - e
        out["var"][F] = np.sum(Lsi * Lsi, axis=0)
        out["mahalanobis"][f] = y @ y
        out["log_score"][f] = -(y @ y) / dt(2) + np.sum(np.log(np.diag(Ls))) - dt(len(F)) / dt(2) * _log_2pi(dt)
    return out


def brute(X, t, theta, labels, k, kernel="SquaredExponential", mean="zero", nugget_fit=False, nugget=None, dtype=np.float64):
    dt = np.dtype(dtype).type
    Q, r, eta = build(X, t, theta, kernel, mean, nugget_fit, nugget, dtype)
    n = Q.shape[0]
    tt = np.asarray(t, dtype=dtype)
    out = {"mean": np.zeros(n, dtype=dtype), "var": np.zeros(n, dtype=dtype), "mahalanobis": np.zeros(k, dtype=dtype),
           "log_score": np.zeros(k, dtype=dtype), "eta": eta}
    every = np.arange(n)
    for f, F in enumerate(_folds(labels, k)):
        R = np.setdiff1d(every, F)
        Li = lower_inverse(cholesky(Q[np.ix_(R, R)]))
        V = Li @ Q[np.ix_(R, F)]
        Sigma = Q[np.ix_(F, F)] - V.T @ V
        e = r[F] - V.T @ (Li @ r[R])
        Lc = cholesky(Sigma)
        z = lower_inverse(Lc) @ e
        out["mean"][F] = tt[F] - e
        out["var"][F] = np.diag(Sigma)
        out["mahalanobis"][f] = z @ z
        out["log_score"][f] = -(z @ z) / dt(2) - np.sum(np.log(np.diag(Lc))) - dt(len(F)) / dt(2) * _log_2pi(dt)
    return out


QUANTITIES = ("mean", "var", "mahalanobis", "log_score")


def disagreement(a, b):
    """largest |a - b| of every quantity relative to the largest entry of b: {name: (relative disagreement, scale)}"""
    out = {}
    for q in QUANTITIES:
        scale = float(np.abs(b[q]).max())
        out[q] = (float(np.abs(a[q] - b[q]).max()) / scale, scale)
    return out


def data(n, D, seed=7):
    """random points in the unit cube, t = sin(3 sum x) + noise"""
    rng = np.random.default_rng(seed + 1000 * n + D)
    X = rng.random((n, D))
    return X, np.sin(3 * X.sum(axis=1)) + 0.05 * rng.standard_normal(n)


def table_case(n, D, k, kernel, eta):
    """a case of the table of the host test: theta = (1, .., 1, 0) (and log eta where the nugget is fitted); k = None is leave-one-out,
    the k-fold labels are arange(n) % k"""
    X, t = data(n, D)
    fit = eta == "fit"
    theta = np.concatenate([np.ones(D), [0.], [-4.] if fit else []])
    labels = np.arange(n) if k is None else np.arange(n) % k
    return X, t, theta, labels, (n if k is None else k), dict(kernel=kernel, nugget_fit=fit, nugget=None if fit else eta)


TABLE = [
    (7, 1, None, "SquaredExponential", 1e-4),
    (33, 1, 3, "SquaredExponential", 1e-4),
    (33, 3, None, "Matern52", "fit"),
    (130, 3, 5, "SquaredExponential", 1e-4),
    (130, 3, 5, "Matern52", "fit"),
    (130, 4, None, "SquaredExponential", 1e-6),
    (257, 4, 2, "Matern52", 1e-4),
    (200, 4, 10, "SquaredExponential", 1e-6),
]
