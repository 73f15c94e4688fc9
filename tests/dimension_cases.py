"""Inputs for the sweep of the input dimension D (test_dimension_cases_host.py, test_gpu_dimension_sweep.py).  Plain NumPy: nothing here
touches the device.

Every coordinate has its own scale (column d of the unit cube is multiplied by 0.5 + d / D) and, for the per-dimension kernels, its own
correlation length, so that a dropped, a repeated or a swapped dimension changes every result.  Theta follows the rule of
test_gpu_parity.py::test_input_dimension_limits -- correlation lengths of 0.3 sqrt(D) -- which keeps K + nugget I well conditioned at
every D (test_dimension_cases_host.py asserts it)."""
from collections import namedtuple

import numpy as np

KERNELS = ["SquaredExponential", "Matern52", "ProductMat52", "UniformSqExp", "UniformMat52"]
PER_DIM = KERNELS[:3]               # one correlation length per input
UNIFORM = KERNELS[3:]               # one correlation length in all
D_SWEEP = [1, 2, 5, 6, 8, 9, 13, 16, 17, 29, 32, 33, 48, 64, 79, 80]
D_EDGES = [16, 17, 32, 33, 80]      # both sides of the two prefetch-depth thresholds of the cross covariance, and the limit
N_TILES = 130                       # three training tiles of 64: the prefetch's double buffer is written, read and reused
N_PARTIAL = 7                       # one partial tile
M_TEST = (37, 65)
NUGGET = 1e-4
LOG_COV = 0.1

Case = namedtuple("Case", "X T Xs thetas kernel nc fit nugget")


def n_corr(kernel, D):
    return 1 if kernel in UNIFORM else D


def column_scale(D):
    return 0.5 + np.arange(D) / D


def theta_of(D, kernel, fit, k=0):
    """[correlation | log sigma^2 | log nugget if fitted] of emulator k"""
    nc = n_corr(kernel, D)
    corr = -2. * np.log(0.3 * np.sqrt(D)) + np.linspace(-0.4, 0.4, nc) + 0.05 * k
    return np.concatenate([corr, [LOG_COV], [np.log(NUGGET)] if fit else []])


def case(n, D, kernel, seed=0, m=M_TEST[0], E=1, fit=False, repeat=False):
    """E emulators on one design.  T is (E, n), thetas (E, n_params); emulator k adds 0.05 k to its correlation parameters and k to its
    targets.  repeat=True makes the last design point a copy of the first, targets included (nugget="pivot" is meant for such designs)."""
    rng = np.random.default_rng([seed, n, D])
    sc = column_scale(D)
    X = rng.random((n, D)) * sc
    Xs = rng.random((m, D)) * sc
    if repeat:
        X[n - 1] = X[0]
    T = np.stack([np.sin(3. * X[:, 0]) + 0.3 * X[:, D - 1] ** 2 + 0.05 * rng.standard_normal(n) + k for k in range(E)])
    if repeat:
        T[:, n - 1] = T[:, 0]
    thetas = np.stack([theta_of(D, kernel, fit, k) for k in range(E)])
    return Case(X, T, Xs, thetas, kernel, n_corr(kernel, D), fit, "fit" if fit else NUGGET)


# The bars of tests/tools/fuzz_parity.py (its close(...) calls), as (rtol, atol) for an amplification of 1; both are multiplied by
# amp = max(1, cond(K + nugget I) * 1e-7), and the gradient's atol also by max(1, max|g|) of the device's gradient.
BARS = {"logpost": (1e-8, 1e-8), "grad": (1e-5, 1e-6), "mean": (1e-6, 1e-7), "var": (1e-5, 1e-8), "deriv": (1e-5, 1e-6),
        "fullcov": (1e-5, 1e-8)}


def amplification(Kn, n_skipped=0):
    """(2-norm condition number over the accepted pivots, the fuzz's amp) of the matrix that is factorised"""
    ev = np.sort(np.linalg.eigvalsh(Kn))[::-1]
    cond = float(ev[0] / max(ev[len(ev) - n_skipped - 1], 1e-300))
    return cond, max(1., cond * 1e-7)


def excess(tag, got, want, amp=1., gscale=1.):
    """largest |got - want| / (atol + rtol |want|) over the entries: <= 1 is what np.allclose accepts at this bar"""
    rtol, atol = BARS[tag]
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    return float(np.max(np.abs(got - want) / (amp * (atol * gscale + rtol * np.abs(want)))))


def oracle(c, k=0, terms=None, X=None, Xs=None, theta=None, deriv=False):
    """log-posterior, gradient, predictive mean, variance (and input derivative) of emulator k on the CPU oracle; X, Xs and theta
    override the case's (the host test removes a column / swaps two parameters through them).  terms: None for a zero mean, else the
    terms of an analytic mean with an intercept.  Returns (dict, fitted oracle object)."""
    from oracle import cpu_ref as R
    X = c.X if X is None else X
    Xs = c.Xs if Xs is None else Xs
    theta = c.thetas[k] if theta is None else theta
    kw = dict(kernel=c.kernel, nugget=c.nugget)
    ref = R.GPRef(X, c.T[k], **kw) if terms is None else R.GPRefMean(X, c.T[k], terms, True, **kw)
    out = {"logpost": ref.fit(theta), "grad": ref.logpost_deriv(theta)}
    out["mean"], out["var"], out["deriv"] = ref.predict(Xs, deriv=deriv)
    return out, ref
