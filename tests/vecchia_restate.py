"""NumPy restatement of the Vecchia likelihood (mogp_emulator_amd.Vecchia), written from the definitions and independent of the package's own
code, in float64 and in np.longdouble.  It builds on local_restate's scales, scaled_r2, kernel_of_r2 and cholesky.

The design X is taken IN THE VECCHIA ORDER: the neighbours c(t) of row t are the min(t, k) smallest pairs (r2, index) over the rows < t in
lexicographic order -- np.lexsort((index, r2)) over the prefix -- with r2 the arithmetic of the contract of include/mogp_hip.h
(local_restate.scaled_r2), so the lists are reproduced bit for bit; -1 behind the neighbours of the first k rows.

Per row, with A = sigma^2 k(r2) + (nugget + jitter) I over (c(t), t) = L L^T, e the last row, z = L^-1 y:
    l_t = -log L_ee - z_e^2 / 2 - log(2 pi) / 2
and, with w = A^-1 e, alpha = A^-1 y, w_e the last entry of w, rho = w^T y, a_p = w^T A_p w, b_p = w^T A_p alpha for A_p = dA / dtheta_p:
    dl_t / dtheta_p = -a_p / (2 w_e) + rho b_p / w_e - rho^2 a_p / (2 w_e^2)
    correlation parameter d:  (A_d)_ij = sigma^2 k'(r2_ij) (x~_id - x~_jd)^2     (the uniform kernels sum over d)
    log sigma^2:  A_p = A - (nugget + jitter) I;      log nugget:  A_p = nugget I
The neighbour lists are an ARGUMENT, so that values can be checked on the device's own lists."""
import numpy as np

import local_restate as lr


def ordered_neighbours(X, s, k):
    """(N, k) int64: row t holds its min(t, k) nearest rows among the rows < t, nearest first, ties to the lowest row; -1 behind them"""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    r2 = lr.scaled_r2(X, X, s)                  # [query, design row]
    nbr = np.full((N, k), -1, dtype=np.int64)
    for t in range(1, N):
        idx = np.lexsort((np.arange(t), r2[t, :t]))[:k]
        nbr[t, :len(idx)] = idx
    return nbr


def kernel_dr2(r2, kind):
    """dk / d(r2)"""
    dtype = r2.dtype.type
    if kind in lr.MATERN:
        sq = np.sqrt(dtype(5) * r2)
        return -(dtype(5) / dtype(6)) * (dtype(1) + sq) * np.exp(-sq)
    return -np.exp(-r2 / dtype(2)) / dtype(2)


def backward(L, B):
    """L^-T B in the dtype of L"""
    V = np.zeros_like(B)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        V[i] = (B[i] - L[i + 1:, i] @ V[i + 1:]) / L[i, i]
    return V


def _log_2pi(dtype):
    return np.log(dtype(8) * np.arctan(dtype(1)))


def _pieces(P, kind, sigma2, dtype):
    """(r2 (n, n), squared differences per dimension (D, n, n)) of scaled points P"""
    diff2 = np.stack([(P[:, d][:, None] - P[:, d][None, :]) ** 2 for d in range(P.shape[1])])
    r2 = np.zeros((P.shape[0], P.shape[0]), dtype=dtype)
    for d in range(P.shape[1]):
        r2 = r2 + diff2[d]
    return r2, diff2


def n_params(D, kind, fit_nugget):
    return (1 if kind in lr.UNIFORM else D) + 1 + (1 if fit_nugget else 0)


def unpack(theta, D, kind, nugget):
    """(s (D,), sigma^2, nugget) of theta = [correlation raws | log sigma^2 | log nugget with nugget="fit"]"""
    theta = np.asarray(theta, dtype=np.float64)
    nc = 1 if kind in lr.UNIFORM else D
    fit = isinstance(nugget, str)
    assert theta.shape == (nc + 1 + (1 if fit else 0),)
    return lr.scales(theta[:nc], D, kind), float(np.exp(theta[nc])), float(np.exp(theta[nc + 1])) if fit else float(nugget)


def _param_grad(a_d, b_d, a_s, b_s, a_n, b_n, we, rho, kind, fit_nugget):
    def entry(a, b):
        return -a / (2 * we) + rho * b / we - rho * rho * a / (2 * we * we)
    corr = [entry(a_d.sum(), b_d.sum())] if kind in lr.UNIFORM else [entry(a, b) for a, b in zip(a_d, b_d)]
    return corr + [entry(a_s, b_s)] + ([entry(a_n, b_n)] if fit_nugget else [])


def terms(X, y, s, kind, sigma2, nugget, nbr, jitter=0., grad=False, fit_nugget=True, dtype=np.float64, rows=None):
    """(terms (N,), gradient rows (N, P) or None, ok (N,) bool, cond (N,) float64) on the lists nbr (N, k), -1 = no neighbour; rows: the rows
    to evaluate (default all; the others stay NaN / False).  A matrix the Cholesky factorisation refuses gives NaN and ok False."""
    X, y, sd = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(s, dtype=dtype)
    N, D = X.shape
    P = n_params(D, kind, fit_nugget)
    out = np.full(N, np.nan, dtype=dtype)
    g = np.full((N, P), np.nan, dtype=dtype) if grad else None
    ok, cond = np.zeros(N, dtype=bool), np.zeros(N)
    da = dtype(nugget) + dtype(jitter)
    for t in (range(N) if rows is None else rows):
        idx = np.r_[np.asarray(nbr[t])[np.asarray(nbr[t]) >= 0], t].astype(int)
        n = len(idx)
        Pt = X[idx] * sd
        r2, diff2 = _pieces(Pt, kind, sigma2, dtype)
        A = dtype(sigma2) * lr.kernel_of_r2(r2, kind) + da * np.eye(n, dtype=dtype)
        ev = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
        cond[t] = float(ev[-1] / max(ev[0], 1e-300))
        try:
            L = lr.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        z = lr.forward(L, y[idx][:, None])[:, 0]
        out[t] = -np.log(L[-1, -1]) - z[-1] * z[-1] / dtype(2) - _log_2pi(dtype) / dtype(2)
        ok[t] = True
        if not grad:
            continue
        e = np.zeros(n, dtype=dtype)
        e[-1] = 1
        w = backward(L, lr.forward(L, e[:, None]))[:, 0]
        alpha = backward(L, z[:, None])[:, 0]
        we, rho = w[-1], w @ y[idx]
        Gm = dtype(sigma2) * kernel_dr2(r2, kind)
        a_d = np.array([w @ (Gm * diff2[d]) @ w for d in range(D)], dtype=dtype)
        b_d = np.array([w @ (Gm * diff2[d]) @ alpha for d in range(D)], dtype=dtype)
        a_s, b_s = we - da * (w @ w), rho - da * (w @ alpha)
        a_n, b_n = dtype(nugget) * (w @ w), dtype(nugget) * (w @ alpha)
        g[t] = _param_grad(a_d, b_d, a_s, b_s, a_n, b_n, we, rho, kind, fit_nugget)
    return out, g, ok, cond


def loglik(X, y, s, kind, sigma2, nugget, nbr, jitter=0., grad=False, fit_nugget=True, dtype=np.float64):
    """(value, gradient (P,) or None) of the Vecchia log-likelihood on the lists nbr"""
    t, g, ok, _ = terms(X, y, s, kind, sigma2, nugget, nbr, jitter, grad, fit_nugget, dtype)
    assert ok.all()
    return t.sum(), (g.sum(axis=0) if grad else None)


def loglik_theta(X, y, theta, kind, nugget, nbr, grad=False, dtype=np.float64):
    """the same as a function of theta (nugget: "fit" or the fixed value)"""
    s, sigma2, nug = unpack(theta, np.shape(X)[1], kind, nugget)
    return loglik(X, y, s, kind, sigma2, nug, nbr, grad=grad, fit_nugget=isinstance(nugget, str), dtype=dtype)


def dense_loglik(X, y, s, kind, sigma2, nugget, grad=False, fit_nugget=True, dtype=np.float64):
    """(log N(y | 0, sigma^2 k + nugget I), its gradient (P,) or None) over the whole design: what the Vecchia sum equals at k = N - 1"""
    X, y, sd = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(s, dtype=dtype)
    N, D = X.shape
    r2, diff2 = _pieces(X * sd, kind, sigma2, dtype)
    A = dtype(sigma2) * lr.kernel_of_r2(r2, kind) + dtype(nugget) * np.eye(N, dtype=dtype)
    L = lr.cholesky(A)
    z = lr.forward(L, y[:, None])[:, 0]
    value = -np.sum(np.log(np.diag(L))) - z @ z / dtype(2) - dtype(N) * _log_2pi(dtype) / dtype(2)
    if not grad:
        return value, None
    alpha = backward(L, z[:, None])[:, 0]
    Ainv = backward(L, lr.forward(L, np.eye(N, dtype=dtype)))
    Gm = dtype(sigma2) * kernel_dr2(r2, kind)

    def entry(Ap):
        return alpha @ Ap @ alpha / dtype(2) - np.sum(Ainv * Ap) / dtype(2)
    per_d = [entry(Gm * diff2[d]) for d in range(D)]
    corr = [np.sum(np.array(per_d, dtype=dtype))] if kind in lr.UNIFORM else per_d
    eye = np.eye(N, dtype=dtype)
    g = corr + [entry(A - dtype(nugget) * eye)] + ([entry(dtype(nugget) * eye)] if fit_nugget else [])
    return value, np.array(g, dtype=dtype)


def draw(X, s, kind, sigma2, nugget, seed):
    """one draw of the zero-mean GP at the rows of X"""
    X = np.asarray(X, dtype=np.float64)
    r2, _ = _pieces(X * s, kind, sigma2, np.float64)
    L = np.linalg.cholesky(sigma2 * lr.kernel_of_r2(r2, kind) + nugget * np.eye(X.shape[0]))
    return L @ np.random.default_rng(seed).standard_normal(X.shape[0])
