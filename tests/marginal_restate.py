"""NumPy restatement of the mixture prediction over hyperparameter samples ("Marginal"), independent of the product: no
import from mogp_emulator_amd.  Everything runs in the dtype asked for -- float64, or np.longdouble for the reference the device tolerance
is derived from -- including the factorisation (a plain Cholesky written here: LAPACK has no long double).

theta = [mean parameters | corr_raw (nc) | log sigma^2 | log eta (fitted nugget only)];  s_p(a, b) = e^{theta_p} (x_ap - x_bp)^2,
r2 = sum_p s_p,  Q = sigma^2 k(r2) + eta I,  alpha = Q^-1 (t - mean(X)).  Per sample
    mu(x*) = mean(x*) + k*^T alpha,   var(x*) = sigma^2 - k*^T Q^-1 k*,   v = max(var + (eta if include_nugget), 0)
    F = 1/2 (t - mean)^T alpha + 1/2 log|Q| + n/2 log 2 pi - log prior(theta)
and over the samples, with normalised weights w_s, the pivot mu_0 (the first sample that factorised) and d_s = mu_s - mu_0:
    mean = mu_0 + sum w_s d_s,   within = sum w_s v_s,   between = max(sum w_s d_s^2 - (sum w_s d_s)^2, 0)

Kernels: "SquaredExponential", "Matern52" (one length per dimension), "UniformSqExp", "UniformMat52" (one shared length).
Mean: "zero", ("fixed", value), "const" (theta[0] is the constant).
"""
import numpy as np

PER_DIM = {"SquaredExponential": "se", "Matern52": "m52"}
UNIFORM = {"UniformSqExp": "se", "UniformMat52": "m52"}


def cholesky(Q):
    """lower Cholesky factor in Q's own dtype; LinAlgError where a pivot is not positive"""
    n = Q.shape[0]
    L = np.zeros_like(Q)
    for j in range(n):
        d = Q[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("matrix is not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (Q[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse(L):
    n = L.shape[0]
    Li = np.zeros_like(L)
    for i in range(n):
        row = -(L[i, :i] @ Li[:i, :])
        row[i] += 1
        Li[i, :] = row / L[i, i]
    return Li


def _kernel(base, r2, dt):
    if base == "se":
        return np.exp(-r2 / dt(2))
    u = np.sqrt(dt(5) * r2)
    return (1 + u + dt(5) / dt(3) * r2) * np.exp(-u)


def n_mean_params(mean):
    return 1 if mean == "const" else 0


def _mean_at(mean, theta, rows, dt):
    if mean == "zero":
        return np.zeros(rows, dtype=dt)
    if mean == "const":
        return np.full(rows, theta[0], dtype=dt)
    return np.full(rows, dt(mean[1]), dtype=dt)


def sample(X, t, theta, Xs, kernel="SquaredExponential", mean="zero", nugget_fit=False, nugget=None, log_prior=None, dtype=np.float64):
    """One hyperparameter sample: (mu (m,), var (m,) raw -- not clipped, no nugget --, F, eta).  nugget_fit: theta ends with log eta;
    otherwise `nugget` is the constant on the diagonal.  log_prior: log prior density at theta (None: weak priors).  Raises LinAlgError
    where Q has no Cholesky factor."""
    dt = np.dtype(dtype).type
    X = np.asarray(X, dtype=dtype)
    Xs = np.asarray(Xs, dtype=dtype)
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
    r2s = (((Xs[:, None, :] - X[None, :, :]) ** 2) * scale).sum(-1)
    Q = sig2 * _kernel(base, r2, dt) + eta * np.eye(n, dtype=dtype)
    L = cholesky(Q)
    Li = lower_inverse(L)
    y = t - _mean_at(mean, theta, n, dt)
    z = Li @ y
    alpha = Li.T @ z
    Ks = sig2 * _kernel(base, r2s, dt)                                   # (m, n)
    mu = _mean_at(mean, theta, Xs.shape[0], dt) + Ks @ alpha
    V = Li @ Ks.T                                                        # (n, m)
    var = sig2 - np.sum(V * V, axis=0)
    F = (z @ z) / dt(2) + np.sum(np.log(np.diag(L))) + dt(n) / dt(2) * np.log(dt(8) * np.arctan(dt(1)))      # 2 pi in the dtype's own precision
    if log_prior is not None:
        F = F - dt(log_prior)
    return mu, var, F, eta


def weights_of(F, ok, weights=None, log_q=None, dtype=np.float64):
    """normalised weights: explicit ones, or exp(-(F - F_a) - (log_q - log_q_a)) with a the first ok sample of the smallest F; samples that
    are not ok get 0; NaN where nothing is left"""
    dt = np.dtype(dtype).type
    ok = np.asarray(ok, dtype=bool)
    S = ok.size
    w = np.zeros(S, dtype=dtype)
    good = np.flatnonzero(ok)
    if good.size == 0:
        return np.full(S, np.nan, dtype=dtype)
    if log_q is not None:
        F = np.asarray(F, dtype=dtype)
        q = np.asarray(log_q, dtype=dtype)
        a = good[np.argmin(F[good])]
        w[good] = np.exp(-(F[good] - F[a]) - (q[good] - q[a]))
    else:
        w[good] = np.asarray(weights, dtype=dtype)[good]
    tot = w.sum()
    if not (tot > 0 and np.isfinite(tot)):
        return np.full(S, np.nan, dtype=dtype)
    return w / tot


def mixture(X, t, thetas, Xs, kernel="SquaredExponential", mean="zero", nugget_fit=False, nuggets=None, weights=None, log_q=None,
            include_nugget=True, log_prior=None, dtype=np.float64):
    """The mixture over the rows of thetas (S, P).  nuggets: per sample, the constant on the diagonal (a scalar for all; ignored with
    nugget_fit); a sample whose entry is None, or whose Q has no Cholesky factor, counts as failed.  log_prior: None or a function of
    theta.  Returns a dict: mean, within, between (m,), weights, F (S,), ok (S,), d2max (the largest d_s^2, the scale of `between`),
    mu, v (S, m) per sample."""
    dt = np.dtype(dtype).type
    thetas = np.asarray(thetas, dtype=np.float64)
    S = thetas.shape[0]
    m = np.asarray(Xs).shape[0]
    if nuggets is None or np.isscalar(nuggets):
        nuggets = [nuggets] * S
    mu = np.full((S, m), np.nan, dtype=dtype)
    v = np.full((S, m), np.nan, dtype=dtype)
    F = np.full(S, np.nan, dtype=dtype)
    ok = np.zeros(S, dtype=bool)
    for s in range(S):
        if not nugget_fit and nuggets[s] is None:
            continue
        try:
            mu[s], var, F[s], eta = sample(X, t, thetas[s], Xs, kernel, mean, nugget_fit, nuggets[s],
                                           None if log_prior is None else log_prior(thetas[s]), dtype)
        except np.linalg.LinAlgError:
            continue
        v[s] = np.maximum(var + (eta if include_nugget else dt(0)), dt(0))
        ok[s] = np.isfinite(F[s])
    w = weights_of(F, ok, weights, log_q, dtype)
    out = {"weights": w, "F": F, "ok": ok, "mu": mu, "v": v}
    nan = np.full(m, np.nan, dtype=dtype)
    if not ok.any() or not np.all(np.isfinite(w)):
        out.update(mean=nan, within=nan.copy(), between=nan.copy(), d2max=dt(0))
        return out
    good = np.flatnonzero(ok)
    mu0 = mu[good[0]]
    d = mu[good] - mu0
    wg = w[good][:, None]
    s1 = np.sum(wg * d, axis=0)
    out.update(mean=mu0 + s1, within=np.sum(wg * v[good], axis=0), between=np.maximum(np.sum(wg * d * d, axis=0) - s1 * s1, dt(0)),
               d2max=np.max(d * d) if d.size else dt(0))
    return out
