"""NumPy restatement of the posterior cross covariance and of the ALC criterion (mogp_emulator_amd.ActiveLearning), written from the
definitions and independent of the package's own code, in float64 and in np.longdouble, with the derived error bars the device is held to.

Fixed hyperparameters theta = [log e_1 .. log e_NC, log sigma^2, (log nugget)], Q = sigma^2 k(X, X) + eta I = L L^T:
    c(x, x') = sigma^2 k(x, x') - k(x)^T Q^-1 k(x'),    s^2(x) = max(c(x, x), 0),
    ALC(c_i) = sum_j w_j c(r_j, c_i)^2 / d_i,           d_i = s^2(c_i) + tau.
Kernels, with r2 = sum_d e_d (x_d - x'_d)^2:
    SquaredExponential  exp(-r2 / 2)                    Matern52      (1 + s + s^2 / 3) exp(-s), s = sqrt(5 r2)
    UniformSqExp        SquaredExponential with one e   ProductMat52  prod_d (1 + s_d + s_d^2 / 3) exp(-s_d), s_d = sqrt(5 e_d (x_d - x'_d)^2)

Bars (first order, 2^-52 = EPS):
    entry:  |dc_ij| <= 4 n EPS cond_2(Q) |k(x_i)|_2 |Q^-1 k(x'_j)|_2 + (D + 4) EPS sigma^2
            -- two backward-stable solves with Q against one another, plus the rounding of the prior term (D products and sums, the
            kernel function, sigma^2, the subtraction);
    ALC:    |dALC_i| <= sum_j w_j (2 |c_ij| dc_ij / d_i + c_ij^2 dd_i / d_i^2),   dd_i = dc_ii.
"""
import numpy as np

EPS = 2. ** -52
KINDS = ("SquaredExponential", "Matern52", "UniformSqExp", "ProductMat52")


def n_corr(kind, D):
    return 1 if kind == "UniformSqExp" else D


def kernel(X1, X2, corr_raw, kind, dtype=np.float64):
    """k(X1, X2) (m1, m2) without sigma^2"""
    X1, X2 = np.asarray(X1, dtype=dtype), np.asarray(X2, dtype=dtype)
    D = X1.shape[1]
    e = np.exp(np.asarray(corr_raw, dtype=dtype))
    if kind == "UniformSqExp":
        e = np.full(D, e[0], dtype=dtype)
    one, five, three, two = dtype(1), dtype(5), dtype(3), dtype(2)
    if kind == "ProductMat52":
        k = np.ones((X1.shape[0], X2.shape[0]), dtype=dtype)
        for d in range(D):
            df = X1[:, d][:, None] - X2[:, d][None, :]
            s = np.sqrt(five * e[d] * df * df)
            k = k * ((one + s + s * s / three) * np.exp(-s))
        return k
    r2 = np.zeros((X1.shape[0], X2.shape[0]), dtype=dtype)
    for d in range(D):
        df = X1[:, d][:, None] - X2[:, d][None, :]
        r2 = r2 + e[d] * df * df
    if kind in ("SquaredExponential", "UniformSqExp"):
        return np.exp(-r2 / two)
    if kind == "Matern52":
        s = np.sqrt(five * r2)
        return (one + s + s * s / three) * np.exp(-s)
    raise ValueError(kind)


def cholesky(Q):
    """lower Cholesky factor in the dtype of Q (np.linalg has no long double)"""
    n = Q.shape[0]
    L = np.zeros_like(Q)
    for j in range(n):
        d = Q[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (Q[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def forward(L, B):
    """L^-1 B in the dtype of L"""
    n = L.shape[0]
    V = np.zeros_like(B)
    for i in range(n):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


class Posterior(object):
    """The posterior of one emulator at fixed hyperparameters: X (n, D), theta as above, eta the nugget in Q"""

    def __init__(self, X, theta, kind, eta, dtype=np.float64):
        self.X, self.kind, self.dtype = np.asarray(X, dtype=dtype), kind, dtype
        self.n, self.D = self.X.shape
        nc = n_corr(kind, self.D)
        self.corr = np.asarray(theta[:nc], dtype=dtype)
        self.sig2 = np.exp(dtype(theta[nc]))
        self.eta = dtype(eta)
        self.Q = self.sig2 * kernel(self.X, self.X, self.corr, kind, dtype) + self.eta * np.eye(self.n, dtype=dtype)
        self.L = cholesky(self.Q)

    def kstar(self, Xs):
        """sigma^2 k(X, Xs) (n, m)"""
        return self.sig2 * kernel(self.X, Xs, self.corr, self.kind, self.dtype)

    def cov(self, X1, X2):
        """c(X1, X2) (m1, m2)"""
        V1, V2 = forward(self.L, self.kstar(X1)), forward(self.L, self.kstar(X2))
        return self.sig2 * kernel(X1, X2, self.corr, self.kind, self.dtype) - V1.T @ V2

    def var(self, Xs):
        """s^2(Xs) (m,), clipped at 0"""
        V = forward(self.L, self.kstar(Xs))
        return np.maximum(self.sig2 - np.sum(V * V, axis=0), self.dtype(0))

    def _bar_parts(self, Xs):
        """(|k(x)|_2, |Q^-1 k(x)|_2) per point, in float64; cond_2(Q) is computed once"""
        if not hasattr(self, "_Q64"):
            self._Q64 = np.asarray(self.Q, dtype=np.float64)
            self.cond = float(np.linalg.cond(self._Q64))
        k = np.asarray(self.kstar(Xs), dtype=np.float64)
        return np.linalg.norm(k, axis=0), np.linalg.norm(np.linalg.solve(self._Q64, k), axis=0)

    def cov_bar(self, X1, X2):
        """the entry bar (m1, m2), in float64"""
        a = self._bar_parts(X1)[0]
        b = self._bar_parts(X2)[1]
        return 4. * self.n * EPS * self.cond * np.outer(a, b) + (self.D + 4) * EPS * float(self.sig2)

    def var_bar(self, Xs):
        """the bar of c(x, x) per point (m,): the diagonal of cov_bar(Xs, Xs)"""
        a, b = self._bar_parts(Xs)
        return 4. * self.n * EPS * self.cond * a * b + (self.D + 4) * EPS * float(self.sig2)


def floor_of(n, sig2):
    return (n + 2) * EPS * float(sig2)


def alc(post, cand, ref, w, tau):
    """(ALC (m_c,), s^2(cand), s^2(ref), degenerate, c(cand, ref) (m_c, m_r), d (m_c,)) of one emulator; the floor rule applied"""
    dt = post.dtype
    C = post.cov(cand, ref)
    sc, sr = post.var(cand), post.var(ref)
    d = sc + dt(tau)
    deg = ~(d > dt(floor_of(post.n, post.sig2)))
    num = (np.asarray(w, dtype=dt)[None, :] * C * C).sum(axis=1)
    out = np.where(deg, dt(0), num / np.where(deg, dt(1), d))
    return out, sc, sr, deg, C, d


def alc_bar(post, cand, ref, w, C, d):
    """the propagated bar (m_c,) in float64: C, d from alc()"""
    C, d = np.asarray(C, dtype=np.float64), np.asarray(d, dtype=np.float64)
    dC = post.cov_bar(cand, ref)
    dd = post.var_bar(cand)
    w = np.asarray(w, dtype=np.float64)
    return (w[None, :] * (2. * np.abs(C) * dC / d[:, None] + C * C * dd[:, None] / d[:, None] ** 2)).sum(axis=1)
