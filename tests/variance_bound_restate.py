"""NumPy restatement of the variance bound of mogp_emulator_amd.IterativeGP (variance_bound, variance_cache), written from the definitions
and independent of the package's own code.

For ANY full-column-rank Q the Galerkin inverse Q (Q^T A Q)^-1 Q^T never exceeds A^-1 (it is A^-1/2 times an orthogonal projector times
A^-1/2), so sigma^2 [+ nugget] - k*^T Q (Q^T A Q)^-1 Q^T k* is never below the exact predictive variance.  With span Q = span L, L the
partial pivoted Cholesky factor of K = sigma^2 k(X, X) that preconditions the solver (iterative_restate.pivoted_cholesky):

  1. G0 = L^T L
  2. G0[:r0, :r0] = C0 C0^T, a PREFIX Cholesky in natural column order, stopped at the first pivot <= tau G0[0, 0], tau = 1e-10
  3. Q = L[:, :r0] C0^-T                                (orthonormal columns)
  4. H = Q^T (A Q), symmetrised as (H + H^T) / 2        (cond H <= cond A: chol(L^T A L) directly would meet cond(A) cond(L)^2)
  5. H[:r, :r] = C C^T, a prefix Cholesky stopped at the first pivot <= 0;  r = var_rank
  6. R = Q[:, :r] C^-T                                  (R^T A R = I)

Both factors are triangular prefixes, so R[:, :r'] is the R of every r' <= r, and the bound at rank r' is
sigma^2 [+ nugget] - sum_{c < r'} (R^T k*)_c^2, floored at zero: a running sum of squares, hence non-increasing in r' bit for bit."""
from collections import namedtuple

import numpy as np

import iterative_restate as ir

TAU = 1e-10

Cache = namedtuple("Cache", "R var_rank r0 Q H L pivots")


def prefix_cholesky(G, floor):
    """(C (r, r) lower triangular, r): G[:r, :r] = C C^T in natural order, stopped at the first pivot that is not above ``floor``"""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    C = np.zeros((n, n))
    for i in range(n):
        for j in range(i):
            C[i, j] = (G[i, j] - C[i, :j] @ C[j, :j]) / C[j, j]
        s = G[i, i] - C[i, :i] @ C[i, :i]
        if not (s > floor and np.isfinite(s)):
            return C[:i, :i], i
        C[i, i] = np.sqrt(s)
    return C, n


def inverse_transposed(C):
    """C^-T of a lower triangular C by substitution on the identity (upper triangular)"""
    r = C.shape[0]
    U = np.zeros((r, r))
    for j in range(r):
        for i in range(j, r):
            U[j, i] = ((1. if i == j else 0.) - C[i, j:i] @ U[j, j:i]) / C[i, i]
    return U


def cache(K, nugget, rank, pivots=None):
    """steps 1-6 on the dense K = sigma^2 k(X, X) (WITHOUT its nugget); pivots: the device's, as iterative_restate.pivoted_cholesky takes them"""
    K = np.asarray(K, dtype=np.float64)
    A = K + nugget * np.eye(K.shape[0])
    L, piv, _ = ir.pivoted_cholesky(K, rank, pivots=pivots)
    G0 = L.T @ L
    C0, r0 = prefix_cholesky(G0, TAU * G0[0, 0])
    Q = L[:, :r0] @ inverse_transposed(C0)
    H = Q.T @ (A @ Q)
    H = 0.5 * (H + H.T)
    C, r = prefix_cholesky(H, 0.)
    R = Q[:, :r] @ inverse_transposed(C)
    return Cache(R, r, r0, Q, H, L, piv)


def profile(R, ks, sigma2, nugget, include_nugget=True):
    """(var_rank + 1, m): row r' the bound of the leading r' columns at the cross covariances ks (N, m); row 0 is the prior variance"""
    base = sigma2 + nugget if include_nugget else sigma2
    w = R.T @ ks
    q = np.vstack([np.zeros((1, ks.shape[1])), np.cumsum(w * w, axis=0)])
    return np.maximum(base - q, 0.)


def bound(R, ks, sigma2, nugget, include_nugget=True, rank=None):
    r = R.shape[1] if rank is None else min(int(rank), R.shape[1])
    return profile(R[:, :r], ks, sigma2, nugget, include_nugget)[r]


def dense_variance(A, ks, sigma2, nugget, include_nugget=True):
    """max(sigma^2 - k*^T A^-1 k* [+ nugget], 0) by a dense solve"""
    v = sigma2 - np.sum(ks * np.linalg.solve(A, ks), axis=0) + (nugget if include_nugget else 0.)
    return np.maximum(v, 0.)
