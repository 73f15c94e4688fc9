"""Host restatements of gKDR's matrix R for the gKDR tests (not part of the package).

R = sum_j G_j^T F G_j with G_j[k, a] = (X_ka - X_ja) Kx_kj / SGX2, F = A^-1 Ky A^-1, A = Kx + N EPS I (the definition of the reference,
DimensionReduction.py:132-236).  `R_direct` evaluates that sum in fp64 with SciPy's Cholesky; `R_exact` evaluates the same R in 80-bit
long double through the identity the device uses (csrc/kernels_gkdr.hip), which is exact algebra, so its error is ~cond(A) * 2^-64.
"""
import sys

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.spatial.distance import pdist, squareform


def scales2(X, Y, X_scale=1.0, Y_scale=1.0, SGX=None, SGY=None):
    """(SGX2, SGY2) as the reference derives them."""
    N = np.shape(X)[0]
    if SGX is None:
        SGX = X_scale * np.median(pdist(X))
    if SGY is None:
        SGY = Y_scale * np.median(pdist(np.reshape(Y, (N, 1))))
    return max(SGX * SGX, sys.float_info.min), max(SGY * SGY, sys.float_info.min)


def R_direct(X, Y, SGX2, SGY2, EPS):
    """fp64: the defining sum, O(N^2 M) memory."""
    X = np.asarray(X, dtype=np.float64)
    N, M = X.shape
    Kx = np.exp(-0.5 * squareform(pdist(X, "sqeuclidean")) / SGX2)
    Ky = np.exp(-0.5 * squareform(pdist(np.reshape(Y, (N, 1)), "sqeuclidean")) / SGY2)
    c = cho_factor(Kx + N * EPS * np.eye(N), lower=True)
    F = cho_solve(c, cho_solve(c, Ky).T).T
    D = (X[:, None, :] - X[None, :, :]) / SGX2              # D[k, j, a] = (X_ka - X_ja) / SGX2
    G = D * Kx[:, :, None]                                    # G[k, j, a] = G_j[k, a]
    FG = np.einsum("kl,lja->kja", F, G)
    return np.einsum("kja,kjb->ab", G, FG)


def _chol_ld(A):
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _inv_spd_ld(A):
    L = _chol_ld(A)
    n = A.shape[0]
    Li = np.zeros_like(A)                                     # L^-1 by forward substitution on the identity
    for i in range(n):
        Li[i, :i + 1] = -(L[i, :i] @ Li[:i, :i + 1])
        Li[i, i] += 1
        Li[i, :i + 1] /= L[i, i]
    return Li.T @ Li


def R_exact(X, Y, SGX2, SGY2, EPS):
    """80-bit long double through s^2 R = Xc^T (F o KxKx) Xc - Xc^T T Xc - (Xc^T T Xc)^T + Xc^T diag(c) Xc."""
    ld = np.longdouble
    X = np.asarray(X, dtype=np.float64).astype(ld)
    N, M = X.shape
    y = np.reshape(np.asarray(Y, dtype=np.float64), (N,)).astype(ld)
    sx, sy = ld(SGX2), ld(SGY2)
    r2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    Kx = np.exp(-r2 / (2 * sx))
    Ky = np.exp(-((y[:, None] - y[None, :]) ** 2) / (2 * sy))
    Ai = _inv_spd_ld(Kx + ld(N) * ld(EPS) * np.eye(N, dtype=ld))
    F = Ai @ Ky @ Ai
    T = Kx * (F @ Kx)
    Xc = X - X.mean(axis=0)
    U = Xc.T @ T @ Xc
    S = Xc.T @ (F * (Kx @ Kx)) @ Xc - U - U.T + (Xc * T.sum(axis=0)[:, None]).T @ Xc
    return S / (sx * sx)


def cond2(X, SGX2, EPS):
    """cond_2(A) of A = Kx + N EPS I (fp64)."""
    N = np.shape(X)[0]
    Kx = np.exp(-0.5 * squareform(pdist(X, "sqeuclidean")) / SGX2)
    w = np.linalg.eigvalsh(Kx + N * EPS * np.eye(N))
    return float(w[-1] / w[0])


def eig_sorted(R):
    """(eigenvalues, B) of R with the reference's call and sort (descending)."""
    L, V = np.linalg.eigh(R)
    idx = np.argsort(L, 0)[::-1]
    return L[idx], V[:, idx]


def check_B(B_dev, B_ref, R_dev, R_ref, eig_ref, min_gap=1e-6):
    """Davis-Kahan: column i of B (up to sign) where the relative eigen-gap g_i >= min_gap: sin(angle) <= 2 |R_dev - R_ref|_2 / gap_i
    + 1e-12.  Returns the number of columns checked."""
    dR = np.linalg.norm(R_dev - R_ref, 2)
    scale = max(np.max(np.abs(eig_ref)), np.finfo(float).tiny)
    checked = 0
    for i in range(B_ref.shape[1]):
        others = np.delete(eig_ref, i)
        if others.size == 0:
            continue
        gap = np.min(np.abs(others - eig_ref[i]))
        if gap / scale < min_gap:
            continue
        # 2 sin(angle / 2) >= sin(angle), without the cancellation of sqrt(1 - cos^2)
        s = min(np.linalg.norm(B_dev[:, i] - B_ref[:, i]), np.linalg.norm(B_dev[:, i] + B_ref[:, i]))
        assert s <= 2 * dR / gap + 1e-12, (i, s, dR, gap)
        checked += 1
    return checked


def lstsq_model(X, Y):
    """A deterministic train_model for tune_parameters: least squares with an intercept on the reduced inputs."""
    A = np.hstack([np.ones((X.shape[0], 1)), X])
    coef = np.linalg.lstsq(A, Y, rcond=None)[0]
    return lambda Z: np.hstack([np.ones((Z.shape[0], 1)), Z]) @ coef
