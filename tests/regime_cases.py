"""Hyperparameter regimes for the covariance paths (test_regime_cases_host.py, test_gpu_regimes.py).  Plain NumPy: nothing here touches the
device.

Every other value test of the suite evaluates the device at correlation lengths of about 0.3 sqrt(D), sigma^2 = e^0.1 and a nugget of 1e-4.
Here the design is fixed -- dimension_cases.case(130, 3, kernel): three tiles, the last partial -- and theta moves to where an optimiser goes:

  name             correlation lengths (units of the cube's edge)        log sigma^2   nugget eta
  base             dimension_cases.theta_of: 0.3 sqrt(D), -+0.4 in theta    0.1          1e-4          the control: today's point
  tail             0.05                                                    0.1          1e-12         SE arguments to 340, every result normal
  underflow        0.02                                                    0.1          1e-4          part of SE's K is subnormal or 0
  needle           theta_corr = 40                                         0.1          1e-4          r2 ~ 1e17: the exponential's clamp; K = sigma^2 I
  long             8                                                       0.1          1e-4          K ~ sigma^2 1 1^T
  ard              (0.05, 0.3 sqrt(D), 60)                                 0.1          1e-4          short, usual, irrelevant
  big_sigma        base                                                    18           1e-4 e^18     targets times e^9
  small_sigma_rel  base                                                   -18           1e-4 e^-18    targets times e^-9
  noise_only       base                                                   -18           1e-4          sigma^2 << eta
  big_nugget       base                                                    0.1          1e2
  twin             base, the last point = the first + 1e-9 in coordinate 0  0.1          1e-4          r2 ~ 1e-17, not 0

ard also runs at D = 17 with 12 of the 17 lengths at 60 (one at 0.05, four at 0.3 sqrt(17)), so the paths that slice D see it.

The long-double references of single entries start from the float64 scaled coordinates u = fl(x s), s = sqrt(exp(theta_d)) in float64, which
is what the device stages; everything behind u is long double (entries)."""
import functools
import math
from collections import namedtuple

import numpy as np

import dimension_cases as dc

LD = np.longdouble
EPS = 2. ** -52
TINY = float(np.finfo(np.float64).tiny)              # the smallest normal double
STEP = 2. ** -1074                                    # the spacing of the subnormal doubles
N, D, M = dc.N_TILES, 3, dc.M_TEST[0]
D_WIDE = 17
NAMES = ("base", "tail", "underflow", "needle", "long", "ard", "big_sigma", "small_sigma_rel", "noise_only", "big_nugget", "twin")
KERNELS = ("SquaredExponential", "Matern52")          # every path
DENSE_KERNELS = KERNELS + ("ProductMat52",)           # the dense value, gradient and predictions
MAY_UNDERFLOW = ("underflow", "needle")               # the only regimes in which an entry of K may lie below the smallest normal double
TWIN_SHIFT = 1e-9

Regime = namedtuple("Regime", "name kernel X t Xs corr log_cov nugget")


def corr_of_length(length):
    """theta of a correlation length: the scaled squared distance is exp(theta) (x - y)^2"""
    return -2. * np.log(np.asarray(length, dtype=np.float64))


def _corr(name, Dn, kernel):
    usual = 0.3 * np.sqrt(Dn)
    if name == "tail":
        return corr_of_length(np.full(Dn, 0.05))
    if name == "underflow":
        return corr_of_length(np.full(Dn, 0.02))
    if name == "needle":
        return np.full(Dn, 40.)
    if name == "long":
        return corr_of_length(np.full(Dn, 8.))
    if name == "ard":
        if Dn == 3:
            return corr_of_length([0.05, usual, 60.])
        assert Dn == D_WIDE
        return corr_of_length([0.05] + [usual] * 4 + [60.] * 12)
    return dc.theta_of(Dn, kernel, False)[:Dn]


_LOG_COV = {"big_sigma": 18., "small_sigma_rel": -18., "noise_only": -18.}
_TARGET_SCALE = {"big_sigma": np.exp(9.), "small_sigma_rel": np.exp(-9.)}


@functools.lru_cache(maxsize=None)
def regime(name, kernel, Dn=D):
    assert name in NAMES and kernel in DENSE_KERNELS
    c = dc.case(N, Dn, kernel, m=M)
    X, t = c.X.copy(), c.T[0] * _TARGET_SCALE.get(name, 1.)
    if name == "twin":
        X[N - 1] = X[0]
        X[N - 1, 0] += TWIN_SHIFT
        t = t.copy()
        t[N - 1] = t[0]
    log_cov = _LOG_COV.get(name, dc.LOG_COV)
    nugget = {"tail": 1e-12, "big_nugget": 1e2, "big_sigma": dc.NUGGET * np.exp(18.), "small_sigma_rel": dc.NUGGET * np.exp(-18.)}.get(name, dc.NUGGET)
    for a in (X, t, c.Xs):
        a.setflags(write=False)
    return Regime(name, kernel, X, t, c.Xs, _corr(name, Dn, kernel), log_cov, float(nugget))


def theta(r, fit):
    """[correlation | log sigma^2 | log nugget if fitted]"""
    return np.concatenate([r.corr, [r.log_cov], [np.log(r.nugget)] if fit else []])


def sigma2(r):
    """exp(log sigma^2) by the C library, as the host code computes it"""
    return math.exp(r.log_cov)


def cases(kernels=KERNELS):
    """(name, kernel, D) of every regime, the wide ard included"""
    return [(n, k, D) for k in kernels for n in NAMES] + [("ard", k, D_WIDE) for k in kernels]


def scales(r):
    """s (D,) float64, as the host hands it to the device"""
    return np.sqrt(np.exp(r.corr))


def scales_libm(r):
    """the same as the dense engine forms it: exp by the C library on the host, then a correctly rounded square root.  (On every regime
    here the two agree bit for bit: test_regime_cases_host.py.)"""
    return np.array([math.sqrt(math.exp(v)) for v in r.corr])


def staged(r, X):
    """u = fl(x s): the float64 scaled coordinates the device stages"""
    return np.asarray(X, dtype=np.float64) * scales(r)


def weights_libm(r):
    """e_d = exp(theta_d) by the C library: the parameter block of the dense engine"""
    return np.array([math.exp(v) for v in r.corr])


def entries(U1, U2, kind, weights=None):
    """(k (n1, n2), gain (n1, n2)) in long double from float64 coordinates: the kernel without sigma^2, and |d log k / d r2| r2, the factor
    by which a relative error of r2 enters k.  r2 = sum_d (u1_d - u2_d)^2 of scaled coordinates, or, with weights e (float64),
    sum_d e_d (x1_d - x2_d)^2 of unscaled ones: the two forms the device has (cov_full_kernel, behind get_K_matrix, stages x unscaled)"""
    U1, U2 = np.asarray(U1, dtype=LD), np.asarray(U2, dtype=LD)
    r2 = np.zeros((U1.shape[0], U2.shape[0]), dtype=LD)
    for d in range(U1.shape[1]):
        t = U1[:, d][:, None] - U2[:, d][None, :]
        r2 = r2 + (t * t if weights is None else LD(weights[d]) * t * t)
    if kind == "Matern52":
        a = np.sqrt(LD(5) * r2)
        poly = LD(1) + a + a * a / LD(3)
        return poly * np.exp(-a), (LD(5) / LD(6)) * (LD(1) + a) / poly * r2
    assert kind == "SquaredExponential", kind
    return np.exp(-r2 / LD(2)), r2 / LD(2)


# Ulps (of 2^-52) a generated entry sigma^2 k may be off by apart from the error of r2: the exponential's 1.3, the product with sigma^2 and
# the rounding of the stored value 1; for the Matern the prefactor 1 + a + (5/3) r2 -- three positive terms, each operation half an ulp,
# (5/3) itself half an ulp -- 2.5 more, and its product with the exponential 0.5.
FIXED_ULPS = {"SquaredExponential": 2.3, "Matern52": 5.3}


def entry_bar(want, gain, kind, Dn):
    """absolute bar per entry of sigma^2 k (want, gain long double): relative FIXED_ULPS + (D + 1) gain ulps; an entry below the smallest
    normal double is also allowed two steps of the subnormal grid"""
    rel = LD(EPS) * (LD(FIXED_ULPS[kind]) + LD(Dn + 1) * gain)
    return rel * np.abs(want) + np.where(np.abs(want) < LD(TINY), LD(2 * STEP), LD(0))


def entry_excess(got, want, gain, kind, Dn):
    """largest |got - want| / bar over the entries (0 / 0 counts as 0: an exact zero where the value is below half a subnormal step)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, bar = np.abs(got.astype(LD) - want), entry_bar(want, gain, kind, Dn)
    frac = np.where(err == 0, LD(0), err / np.where(bar > 0, bar, LD(STEP) * LD(STEP)))
    return float(np.max(frac))


# ---- references, computed once per process and shared; never modified ------------------------------------------------------------------------
K_LOCAL = 30


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def dense_reference(name, kernel, Dn=D, dtype=LD):
    """the dense restatement with the nugget as a parameter (a fixed nugget is the same model: its gradient is this one without the last
    entry): logpost and grad in the package's sign, mean, var, deriv, fullcov at the 37 queries, and cond of the float64 matrix"""
    import dense_restate as dr
    import local_restate as lr
    r = regime(name, kernel, Dn)
    m = dr.Dense(r.X, r.t, theta(r, True), kernel, "fit", dtype)
    out = dict(logpost=-m.loglik(), grad=-m.grad(), **m.predict(r.Xs))
    out["A"] = m.A
    Ks = m.sigma2 * dr.kernel(m.U, np.asarray(r.Xs, dtype=dtype) * m.s, kernel, dtype)[0]
    W = dr.backward(m.L, lr.forward(m.L, Ks))
    out["wnorm"] = np.sqrt(np.sum(W * W, axis=0))                    # |A^-1 k*| per query: what a residual of alpha reaches the mean through
    out["cond"], out["amp"] = dc.amplification(np.asarray(m.A, dtype=np.float64))
    return _freeze(out)


def needle_closed_form(r):
    """the dense quantities of K = sigma^2 I in long double: what the needle regime must give whatever the kernel"""
    n, Dn, m = r.X.shape[0], r.X.shape[1], r.Xs.shape[0]
    s2, eta, y = np.exp(LD(r.log_cov)), LD(r.nugget), np.asarray(r.t, dtype=LD)
    a, yy = s2 + eta, y @ y
    loglik = -LD(n) / 2 * np.log(a) - yy / (2 * a) - LD(n) / 2 * np.log(LD(8) * np.arctan(LD(1)))
    dla = yy / (2 * a * a) - LD(n) / (2 * a)
    grad = np.array([LD(0)] * Dn + [s2 * dla, eta * dla], dtype=LD)
    return dict(logpost=-loglik, grad=-grad, mean=np.zeros(m, dtype=LD), var=np.full(m, a, dtype=LD), deriv=np.zeros((m, Dn), dtype=LD),
                fullcov=a * np.eye(m, dtype=LD))


def local_reference(r, nbr, dtype=LD):
    """(mean, var, ok, cond) of local_restate.predict on the lists nbr"""
    import local_restate as lr
    return lr.predict(r.X, r.t, r.Xs, scales(r), r.kernel, sigma2(r), r.nugget, nbr, dtype=dtype)


def vecchia_reference(r, nbr, dtype=LD):
    """(terms, gradient rows, ok, cond) of vecchia_restate.terms in the identity order on the lists nbr, the nugget a parameter"""
    import vecchia_restate as vr
    return vr.terms(r.X, r.t, scales(r), r.kernel, sigma2(r), r.nugget, nbr, grad=True, fit_nugget=True, dtype=dtype)


HESSIAN_MARGIN = CV_MARGIN = 100.
ILL = 1e-8                                            # test_gpu_hessian.py, test_gpu_cv.py: a larger float64 / long double disagreement judges no kernel


@functools.lru_cache(maxsize=None)
def hessian_reference(name, kernel, Dn, fit):
    """dict(H float64 restatement, HL long double, scale = max|HL|, dis = their disagreement relative to scale, floored = dis below n 2^-52,
    bar = 100 max(dis, n 2^-52) scale).  Weak priors, as everywhere in these regimes."""
    import hessian_restate as hr
    r = regime(name, kernel, Dn)
    args = (r.X, r.t, theta(r, fit), kernel, fit, None if fit else r.nugget, None)
    H, HL = hr.hessian(*args), hr.hessian(*args, dtype=LD)
    scale = float(np.abs(HL).max())
    dis = float(np.abs(H - HL).max()) / scale
    floor = r.X.shape[0] * EPS
    return _freeze(dict(H=H, HL=HL, scale=scale, dis=dis, floored=dis < floor, bar=HESSIAN_MARGIN * max(dis, floor) * scale))


CV_FOLDS = 5


@functools.lru_cache(maxsize=None)
def cv_reference(name, kernel, Dn, k):
    """(float64 restatement, long double restatement) of cv_restate.fast; k None: leave-one-out, else labels arange(n) % k"""
    import cv_restate as cr
    r = regime(name, kernel, Dn)
    n = r.X.shape[0]
    labels = np.arange(n) if k is None else np.arange(n) % k
    args = (r.X, r.t, theta(r, False), labels, n if k is None else k, kernel, "zero", False, r.nugget)
    return cr.fast(*args), cr.fast(*args, dtype=LD)


def cv_disagreement(r, a, b):
    """cv_restate.disagreement: every quantity relative to its largest entry.  In `needle` the leave-out mean t_i - e_i is identically 0 (K is
    diagonal) and its largest entry is rounding noise, so there the mean is measured against max|t|, the size of the two terms it is the
    difference of."""
    import cv_restate as cr
    out = cr.disagreement(a, b)
    if r.name == "needle":
        scale = float(np.abs(r.t).max())
        out["mean"] = (float(np.abs(a["mean"] - b["mean"]).max()) / scale, scale)
    return out


ITER_RANK, ITER_RTOL, ITER_MAX, ITER_CAP = 32, 1e-10, 1000, 600      # test_iterative_host.py's tolerance, limit and cap; the rank of its n = 130 shapes


def exact_mean_bar(ref, r, alpha):
    """the bar of test_gpu_iterative.py for the mean of an iterative solve: BARS["mean"] and, for an inexact alpha, |A^-1 k*| |y - A alpha|
    (exact algebra); everything in long double from the dense reference ref"""
    rt, at = dc.BARS["mean"]
    res = np.asarray(r.t, dtype=LD) - ref["A"] @ np.asarray(alpha, dtype=LD)
    return ref["amp"] * (at + rt * np.abs(ref["mean"])) + ref["wnorm"] * np.sqrt(res @ res)
