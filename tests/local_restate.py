"""NumPy restatement of local approximate GP prediction (mogp_emulator_amd.LocalGP), written from the definitions and independent of the
package's own code, in float64 and in np.longdouble.

Neighbour search -- the contract of include/mogp_hip.h, reproduced bit for bit in float64: s_d = sqrt(exp(theta_d)) (one shared value for the
uniform kernels), x~ = x_d * s_d and q~ = q_d * s_d (one rounded multiply each), r2 = ((0 + t_0 t_0) + t_1 t_1) + ... with t_d = x~_d - q~_d
in the order d = 0 .. D-1, every operation a ufunc of its own (NumPy never fuses a multiply into an add); the neighbours of a query are the k
smallest pairs (r2, index) in lexicographic order: np.lexsort((index, r2)).

Values -- per query the dense GP on its neighbours: Q = sigma^2 k(r2) + (nugget + jitter) I = L L^T, z = L^-1 y, v = L^-1 k*,
mean = z . v, variance = max(sigma^2 - v . v + (nugget if include_nugget), 0).  The neighbour lists are an ARGUMENT, so that values can be
checked on the device's own lists.  Kernels of the scaled squared distance: SquaredExponential / UniformSqExp exp(-r2 / 2),
Matern52 / UniformMat52 (1 + s + s^2 / 3) exp(-s) with s = sqrt(5 r2)."""
import numpy as np

UNIFORM = ("UniformSqExp", "UniformMat52")
MATERN = ("Matern52", "UniformMat52")


def scales(corr_raw, D, kind):
    """s (D,) float64 as the host hands it to the device"""
    s = np.sqrt(np.exp(np.asarray(corr_raw, dtype=np.float64)))
    return np.full(D, s[0]) if kind in UNIFORM else s


def scaled_r2(X, Q, s):
    """(m, N) scaled squared distances, the arithmetic of the contract"""
    Xt, Qt = np.asarray(X, dtype=np.float64) * s, np.asarray(Q, dtype=np.float64) * s
    r2 = np.zeros((Qt.shape[0], Xt.shape[0]))
    for d in range(Xt.shape[1]):
        t = Xt[None, :, d] - Qt[:, d, None]
        r2 = r2 + t * t
    return r2


def neighbours(X, Q, s, k):
    """(indices (m, k) int64 nearest first, radius (m,), r2 (m, N))"""
    r2 = scaled_r2(X, Q, s)
    index = np.arange(r2.shape[1])
    nbr = np.stack([np.lexsort((index, row))[:k] for row in r2]).astype(np.int64)
    return nbr, r2[np.arange(r2.shape[0]), nbr[:, -1]], r2


def kernel_of_r2(r2, kind):
    dtype = r2.dtype.type
    if kind in MATERN:
        sq = np.sqrt(dtype(5) * r2)
        return (dtype(1) + sq + sq * sq / dtype(3)) * np.exp(-sq)
    return np.exp(-r2 / dtype(2))


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
    V = np.zeros_like(B)
    for i in range(L.shape[0]):
        V[i] = (B[i] - L[i, :i] @ V[:i]) / L[i, i]
    return V


def _pair_r2(A, B):
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=A.dtype)
    for d in range(A.shape[1]):
        t = A[:, d][:, None] - B[:, d][None, :]
        r2 = r2 + t * t
    return r2


def local_matrix(X, s, kind, sigma2, diag, idx, dtype=np.float64):
    """Q of one query: sigma^2 k + diag I over the design rows idx"""
    P = np.asarray(X, dtype=dtype)[idx] * np.asarray(s, dtype=dtype)
    return dtype(sigma2) * kernel_of_r2(_pair_r2(P, P), kind) + dtype(diag) * np.eye(len(idx), dtype=dtype)


def predict(X, y, Q, s, kind, sigma2, nugget, nbr, jitter=0., include_nugget=True, dtype=np.float64):
    """(mean (m,), variance (m,), ok (m,) bool, cond (m,) float64 2-norm condition number of every local matrix) on the lists nbr (m, k);
    a matrix the Cholesky factorisation refuses gives NaN and ok False"""
    X, y, Q = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(Q, dtype=dtype)
    sd = np.asarray(s, dtype=dtype)
    m = Q.shape[0]
    mean, var = np.full(m, np.nan, dtype=dtype), np.full(m, np.nan, dtype=dtype)
    ok, cond = np.zeros(m, dtype=bool), np.zeros(m)
    for j in range(m):
        idx = np.asarray(nbr[j])
        P = X[idx] * sd
        Kq = dtype(sigma2) * kernel_of_r2(_pair_r2(P, P), kind) + dtype(nugget + jitter) * np.eye(len(idx), dtype=dtype)
        ks = dtype(sigma2) * kernel_of_r2(_pair_r2(P, (Q[j] * sd)[None, :]), kind)[:, 0]
        ev = np.linalg.eigvalsh(np.asarray(Kq, dtype=np.float64))
        cond[j] = float(ev[-1] / max(ev[0], 1e-300))
        try:
            L = cholesky(Kq)
        except np.linalg.LinAlgError:
            continue
        zv = forward(L, np.stack([y[idx], ks], axis=1))
        mean[j] = zv[:, 0] @ zv[:, 1]
        v = dtype(sigma2) - zv[:, 1] @ zv[:, 1] + (dtype(nugget) if include_nugget else dtype(0))
        var[j] = v if v > 0 else dtype(0)
        ok[j] = True
    return mean, var, ok, cond
