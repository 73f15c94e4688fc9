"""NumPy restatement of the variance-based sensitivity estimators the device computes (mogp_emulator_amd/SensitivityAnalysis.py), from
given model evaluations; a helper for test_sobol_host.py and test_gpu_sobol.py, not a test.

A, B: two independent (N, D) sample matrices; AB_i: A with column i taken from B; fA = f(A), fB = f(B), fAB[i] = f(AB_i):

    f0   = mean(concat(fA, fB))
    V    = mean((concat(fA, fB) - f0)**2)                 two passes, population variance
    S_i  = mean((fB - f0) * (fAB_i - fA)) / V             first order, Saltelli et al. 2010
    ST_i = mean((fA - fAB_i)**2) / (2 V)                  total effect, Jansen 1999
"""
import numpy as np


def pick_freeze(A, B, i):
    """AB_i: a copy of A whose column i is B's."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    assert A.shape == B.shape and A.ndim == 2 and 0 <= i < A.shape[1]
    out = A.copy()
    out[:, i] = B[:, i]
    return out


def all_points(A, B):
    """The (D + 2) N points of one analysis in the order A, B, AB_0, ..., AB_{D-1}."""
    return np.concatenate([A, B] + [pick_freeze(A, B, i) for i in range(A.shape[1])], axis=0)


def split_points(f, N, D):
    """fA (..., N), fB (..., N), fAB (..., D, N) from the values f (..., (D + 2) N) at all_points."""
    f = np.asarray(f)
    fA, fB = f[..., :N], f[..., N:2 * N]
    fAB = f[..., 2 * N:].reshape(f.shape[:-1] + (D, N))
    return fA, fB, fAB


def sobol_restate(fA, fB, fAB):
    """fA, fB (..., N), fAB (..., D, N) -> dict(first_order (..., D), total (..., D), mean (...), variance (...)).  V == 0 gives NaN
    indices."""
    fA, fB, fAB = (np.asarray(a, dtype=np.float64) for a in (fA, fB, fAB))
    assert fA.shape == fB.shape and fAB.shape == fA.shape[:-1] + (fAB.shape[-2], fA.shape[-1])
    both = np.concatenate([fA, fB], axis=-1)
    f0 = np.mean(both, axis=-1)
    V = np.mean((both - f0[..., None]) ** 2, axis=-1)
    num_s = np.mean((fB - f0[..., None])[..., None, :] * (fAB - fA[..., None, :]), axis=-1)
    num_t = np.mean((fA[..., None, :] - fAB) ** 2, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Vd = np.where(V > 0., V, np.nan)[..., None]
        S = num_s / Vd
        ST = num_t / (2. * Vd)
    return dict(first_order=S, total=ST, mean=f0, variance=V)


def ishigami(X, a=7., b=0.1):
    X = np.asarray(X, dtype=np.float64)
    return np.sin(X[:, 0]) + a * np.sin(X[:, 1]) ** 2 + b * X[:, 2] ** 4 * np.sin(X[:, 0])


def ishigami_exact(a=7., b=0.1):
    """Analytic first-order and total-effect indices of the Ishigami function on [-pi, pi]^3."""
    pi = np.pi
    V = a * a / 8. + b * pi ** 4 / 5. + b * b * pi ** 8 / 18. + 0.5
    V1 = 0.5 * (1. + b * pi ** 4 / 5.) ** 2
    V2 = a * a / 8.
    V13 = b * b * pi ** 8 * (1. / 18. - 1. / 50.)
    return np.array([V1, V2, 0.]) / V, np.array([V1 + V13, V2, V13]) / V
