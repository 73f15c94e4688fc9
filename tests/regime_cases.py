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


# ---- the analyses (test_regime_analyses_host.py, test_gpu_regime_analyses.py) ------------------------------------------------------------------
# Ulps (of 2^-52) an entry 2 s_d sigma^2 k'(r2) (q~_d - x~_d) of the input-derivative sweep (kinderiv_kernel behind a unit vector: the MFMA adds
# one product with 1 and zeros, which is exact) may be off by apart from the error of r2, read off kern_dr2 and the kernel's text: the table
# exponential 1.3; the product with sigma^2, the rounded difference q~_d - x~_d, its product with g, and the product with 2 s_d in the store
# (2 s_d itself is exact) half an ulp each: 3.3.  The squared exponential's -0.5 is a power of two.  For the Matern 1 + t, the constant 5/6,
# its product with 1 + t and the product with the exponential add half an ulp each: 5.3.  (The two roundings of t = sqrt(5 r2) enter through
# the gain and sit in the (D + 1) of the bar, as for k.)
FIXED_ULPS_DR2 = {"SquaredExponential": 3.3, "Matern52": 5.3}
ANALYSIS_SEED = 20264                                 # candidates and reference points: the first seed from 20261 on at which every candidate of `underflow` lies close enough to a
                                                      # reference point for alc_bar / ALC < 0.05 there (a premise about the inputs, checked on the CPU: test_regime_analyses_host.py)
N_CAND, N_REF, N_FAR_B, FAR_LENGTHS = 129, 130, 64, 300.
N_SHARED = 5                                          # reference points appended to the candidates in `needle`


def entries_dr2(U1, U2, kind):
    """(k' (n1, n2) = dk / dr2 without sigma^2, gain' = |d log|k'| / d r2| r2, the differences (D, n1, n2), the exponential alone) in long double
    from float64 scaled coordinates"""
    U1, U2 = np.asarray(U1, dtype=LD), np.asarray(U2, dtype=LD)
    diff = np.stack([U1[:, d][:, None] - U2[:, d][None, :] for d in range(U1.shape[1])])
    r2 = np.zeros(diff.shape[1:], dtype=LD)
    for d in range(diff.shape[0]):
        r2 = r2 + diff[d] * diff[d]
    if kind == "Matern52":
        a = np.sqrt(LD(5) * r2)
        return -(LD(5) / LD(6)) * (LD(1) + a) * np.exp(-a), LD(5) * r2 / (LD(2) * (LD(1) + a)), diff, np.exp(-a)
    assert kind == "SquaredExponential", kind
    return -np.exp(-r2 / LD(2)) / LD(2), r2 / LD(2), diff, np.exp(-r2 / LD(2))


@functools.lru_cache(maxsize=None)
def deriv_entries(name, kernel, Dn, on_design):
    """(want (m, D, N) long double, bar, literal bar): G[i, d, j] = 2 s_d sigma^2 k'(r2_ij) (q~_id - x~_jd) at the 37 queries or at the design
    itself.  The literal bar is 2^-52 (FIXED_ULPS_DR2 + (D + 1) gain') |want|, two subnormal steps more where |want| lies below the smallest
    normal double.  It cannot be met by float64 arithmetic that forms g = sigma^2 k' before the product with the difference and with 2 s_d, as
    the kernel and the restatement both do: where the exponential, its half or g is itself subnormal, each of the three carries half a step
    of the subnormal grid, and the later factors multiply that: with e the exponential, h = e / 2 (the Matern: (5/6)(1 + t) e, bounded the
    same way with sigma^2 (5/6)(1 + t) in sigma^2's place) and g = sigma^2 h the errors in steps are 0.5, 0.75, 0.75 sigma^2 + 0.5, then
    |q~_d - x~_d| times that plus 0.5 for the product, and 2 s_d times that plus 0.5 for the store.  In `underflow` 2 s_d |q~_d - x~_d| reaches
    5e3, and the float64 restatement sits at 2e3 times the literal bar (test_regime_analyses_host.py asserts that it does, so that this
    paragraph cannot go stale).  The bar used is therefore the literal one with, where e / 2 or g lies below the smallest normal double,
    the carried steps in place of the two:  2^-1074 [2 s_d (|q~_d - x~_d| (0.75 c + 0.5) + 0.5) + 0.5],  c = sigma^2 (Matern: sigma^2 (5/6)(1 + t))."""
    r = regime(name, kernel, Dn)
    U = staged(r, r.X)
    kd, gain, diff, expo = entries_dr2(U if on_design else staged(r, r.Xs), U, kernel)
    s, s2 = scales(r), LD(sigma2(r))
    want = np.stack([LD(2) * LD(s[d]) * s2 * kd * diff[d] for d in range(Dn)], axis=1)
    rel = (LD(EPS) * (LD(FIXED_ULPS_DR2[kernel]) + LD(Dn + 1) * gain))[:, None, :] * np.abs(want)
    literal = rel + np.where(np.abs(want) < LD(TINY), LD(2 * STEP), LD(0))
    c = s2 * np.abs(kd) / np.where(expo > 0, expo, LD(1)) * (LD(2) if kernel == "SquaredExponential" else LD(1))
    low = np.minimum(expo / 2, s2 * np.abs(kd)) < LD(TINY)
    carried = np.stack([LD(STEP) * (LD(2) * LD(s[d]) * (np.abs(diff[d]) * (LD(0.75) * c + LD(0.5)) + LD(0.5)) + LD(0.5)) for d in range(Dn)], axis=1)
    bar = np.where(low[:, None, :], rel + np.maximum(carried, LD(2 * STEP)), literal)
    for a in (want, bar, literal):
        a.setflags(write=False)
    return want, bar, literal


def excess(got, want, bar):
    """largest |got - want| / bar, the difference in long double; an exact agreement counts as 0 whatever the bar"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got.astype(LD) - want)
    bar = np.asarray(bar, dtype=LD)
    return float(np.max(np.where(err == 0, LD(0), err / np.where(bar > 0, bar, LD(STEP) * LD(STEP)))))


@functools.lru_cache(maxsize=None)
def point_sets(name, kernel, Dn=D):
    """dict(cand (129, D), ref (130, D): the 37 queries and 93 more, far_a (37, D), far_b (64, D)): candidates and reference points uniform in
    the design's bounding box; the far sets are the queries and the first 64 candidates moved by 300 correlation lengths in every coordinate"""
    r = regime(name, kernel, Dn)
    rng = np.random.default_rng(ANALYSIS_SEED)
    lo, hi = r.X.min(axis=0), r.X.max(axis=0)
    cand = lo + (hi - lo) * rng.random((N_CAND, Dn))
    more = lo + (hi - lo) * rng.random((N_REF - r.Xs.shape[0], Dn))
    shift = FAR_LENGTHS / scales(r)
    return _freeze(dict(cand=cand, ref=np.vstack([r.Xs, more]), far_a=r.Xs + shift, far_b=cand[:N_FAR_B] + shift))


@functools.lru_cache(maxsize=None)
def far_reference(name, kernel, Dn=D):
    """dict(kstar: the largest long-double entry of k between the far sets and the design; ab, aa: (want, gain) of sigma^2 k(far_a, far_b) and
    sigma^2 k(far_a, far_a) from the staged coordinates)"""
    r, ps = regime(name, kernel, Dn), point_sets(name, kernel, Dn)
    U, A, B = staged(r, r.X), staged(r, ps["far_a"]), staged(r, ps["far_b"])
    kstar = max(entries(A, U, kernel)[0].max(), entries(B, U, kernel)[0].max())          # long double: 2^-1080 is no float64
    out = dict(kstar=kstar)
    for tag, V in (("ab", B), ("aa", A)):
        k, gain = entries(A, V, kernel)
        out[tag] = (LD(sigma2(r)) * k, gain)
    return out


@functools.lru_cache(maxsize=None)
def posterior(name, kernel, Dn=D, dtype=LD):
    """alc_restate.Posterior of the regime, the nugget a parameter of theta or fixed: the same model"""
    import alc_restate as ar
    r = regime(name, kernel, Dn)
    return ar.Posterior(r.X, theta(r, False), kernel, r.nugget, dtype)


@functools.lru_cache(maxsize=None)
def alc_reference(name, kernel, Dn=D, dtype=LD):
    """dict(C (129, 130), cbar, alc (129,), abar, deg, sc, sr) of the general case, uniform weights, tau = the nugget"""
    import alc_restate as ar
    r, ps, p = regime(name, kernel, Dn), point_sets(name, kernel, Dn), posterior(name, kernel, Dn, dtype)
    w = np.full(N_REF, 1. / N_REF)
    a, sc, sr, deg, C, d = ar.alc(p, ps["cand"], ps["ref"], w, r.nugget)
    return _freeze(dict(C=C, cbar=p.cov_bar(ps["cand"], ps["ref"]), alc=a, abar=ar.alc_bar(p, ps["cand"], ps["ref"], w, C, d), deg=deg, sc=sc, sr=sr))


PATH_SEED, PATH_STREAM, PATH_F, PATH_S = 11, 0x200, 130, 3


@functools.lru_cache(maxsize=None)
def feature_reference(name, kernel, Dn=D):
    """dict(omega, phase, W, amp, arg: the largest |argument|, val (37, 3), vbar, grad (37, D, 3), gbar, scale: amp sum_f |W_sf| (3,)) of the feature
    product and its derivative at the staged queries in long double"""
    import inputderiv_restate as idr
    import pathwise_restate as pw
    from mogp_emulator_amd.Sampling import philox_normals
    r = regime(name, kernel, Dn)
    omega, phase = pw.features(PATH_SEED, PATH_STREAM, PATH_F, Dn, kernel)
    W = philox_normals(PATH_SEED, PATH_STREAM + 3, PATH_S, PATH_F)
    Pt, s, s2 = staged(r, r.Xs), scales(r), sigma2(r)
    amp = float(np.sqrt(2. * s2 / PATH_F))
    return _freeze(dict(omega=omega, phase=phase, W=W, amp=amp, arg=float(np.abs(pw.arguments(Pt, omega, phase)).max()),
                        val=pw.rff(Pt, omega, phase, W, s2, LD), vbar=pw.rff_bar(Pt, omega, phase, W, s2),
                        grad=idr.rff_grad(Pt, s, omega, phase, W, s2, LD), gbar=idr.rffgrad_bar(Pt, s, omega, phase, W, s2),
                        scale=amp * np.abs(W).sum(axis=1)))


BATCH_Q = 6
TIGHT = ("tail", "underflow", "noise_only", "big_nugget")            # the regimes in which alc_bar is a few ulps of the score
GAP = 20.                                             # top-two gap, in bars, from which a greedy pick is pinned


@functools.lru_cache(maxsize=None)
def batch_reference(name, kernel, Dn=D):
    """alc_batch_restate.greedy(route="fresh") of the regime: q = 6, select "each", uniform weights, tau = the nugget, no pending points"""
    import alc_batch_restate as br
    r, ps = regime(name, kernel, Dn), point_sets(name, kernel, Dn)
    return br.greedy(r.X, [theta(r, False)], kernel, [r.nugget], ps["cand"], ps["ref"], np.full(N_REF, 1. / N_REF), [r.nugget], BATCH_Q)


@functools.lru_cache(maxsize=None)
def batch_steps(name, kernel, Dn, picks):
    """the fresh route on a GIVEN history (picks: a tuple of candidate indices): dict(alc (q, m_c), bar (q, m_c): step t scored on the posterior
    of the design with picks[:t] appended at noise tau; iv (q + 1,), iv_bar (q + 1,))"""
    import alc_batch_restate as br
    import alc_restate as ar
    r, ps = regime(name, kernel, Dn), point_sets(name, kernel, Dn)
    w, q = np.full(N_REF, 1. / N_REF), len(picks)
    out = dict(alc=np.zeros((q, N_CAND)), bar=np.zeros((q, N_CAND)), iv=np.zeros(q + 1), iv_bar=np.zeros(q + 1))
    for t in range(q + 1):
        post = br.Augmented(r.X, theta(r, False), kernel, r.nugget, ps["cand"][list(picks[:t])], r.nugget)
        a, _, sr, _, C, d = ar.alc(post, ps["cand"], ps["ref"], w, r.nugget)
        out["iv"][t], out["iv_bar"][t] = float(sr @ w), float(post.var_bar(ps["ref"]) @ w)
        if t < q:
            out["alc"][t], out["bar"][t] = a, ar.alc_bar(post, ps["cand"], ps["ref"], w, C, d)
    return _freeze(out)


def path_normals():
    """(W (3, 130), eps (3, N)) of the paths: the caller's normals, the same in every regime"""
    rng = np.random.default_rng([PATH_SEED, N, PATH_S, PATH_F])
    return rng.standard_normal((PATH_S, PATH_F)), rng.standard_normal((PATH_S, N))


def path_truth(r, omega, phase, W, update, dtype=LD):
    """(value (S, m), its bar, gradient (S, m, D), its bar) of paths at the 37 queries from the fields a PosteriorPaths holds -- the frequencies,
    phases and weights of the prior and the update v (N, S) as they are: no solve here.  Values in `dtype`; the bars are those of
    test_gpu_pathwise.py and test_gpu_inputderiv.py: the two products' (rff_bar; a fixed-order sum of N generated entries times v:
    2^-52 [(N + 4) |K| |v| + (4 D + 32) sigma^2 sum |v|], test_iterative_host.matvec_bar with this regime's sigma^2; rffgrad_bar, kgrad_bar)
    and the rounding of the sums"""
    import inputderiv_restate as idr
    import iterative_restate as ir
    import pathwise_restate as pw
    s, s2, Dn = scales(r), sigma2(r), r.X.shape[1]
    Qt, Xt = staged(r, r.Xs), staged(r, r.X)
    K = ir.covariance(r.Xs, r.X, s, r.kernel, s2, dtype)
    val = (pw.rff(Qt, omega, phase, W, s2, dtype) + K @ np.asarray(update, dtype=np.float64).astype(dtype)).T
    K64, v64 = np.abs(np.asarray(K, dtype=np.float64)), np.abs(np.asarray(update, dtype=np.float64))
    vbar = (pw.rff_bar(Qt, omega, phase, W, s2) + EPS * ((N + 4) * (K64 @ v64) + (4 * Dn + 32) * s2 * v64.sum(axis=0)[None, :])).T \
        + EPS * np.abs(np.asarray(val, dtype=np.float64))
    prior = np.transpose(idr.rff_grad(Qt, s, omega, phase, W, s2, dtype), (2, 0, 1))
    grad = idr.path_gradient(r.X, r.Xs, s, r.kernel, s2, omega, phase, W, update, dtype=dtype)
    gbar = (np.transpose(idr.rffgrad_bar(Qt, s, omega, phase, W, s2), (2, 0, 1)) + EPS * np.abs(np.asarray(prior, dtype=np.float64))
            + np.transpose(idr.kgrad_bar(Qt, Xt, s, r.kernel, s2, update), (2, 0, 1)) + EPS * np.abs(np.asarray(grad, dtype=np.float64)))
    return val, vbar, grad, gbar


def deriv_bar(ref, r, alpha, name, kernel, Dn):
    """the bar of test_gpu_inputderiv.py for d mean / dx of an iterative solve: BARS["deriv"] and, for an inexact alpha,
    |A^-1 d_d k*| |y - A alpha| (exact algebra), d_d k* the entries of deriv_entries; as exact_mean_bar"""
    rt, at = dc.BARS["deriv"]
    res = np.asarray(r.t, dtype=LD) - ref["A"] @ np.asarray(alpha, dtype=LD)
    dk = np.asarray(deriv_entries(name, kernel, Dn, False)[0], dtype=np.float64)                   # (m, D, N)
    W = np.linalg.solve(np.asarray(ref["A"], dtype=np.float64), dk.reshape(-1, dk.shape[2]).T)      # (N, m D)
    wn = np.sqrt(np.sum(W * W, axis=0)).reshape(dk.shape[:2])
    return ref["amp"] * (at + rt * np.abs(ref["deriv"])) + wn * float(np.sqrt(res @ res))


# ---- mixtures and joint draws ------------------------------------------------------------------------------------------------------------------
MIX_NAMES = tuple(n for n in NAMES if n != "twin")    # the regimes on the shared design: the samples of one emulator
MIX_MARGIN, MIX_WEIGHTS = 100., ("uniform", "dirichlet")
DRAWS = 3


def mixture_thetas(kernel):
    """(10, D + 2): theta(regime(name), fit=True) of every regime but `twin` -- samples of one emulator that differ by 36 in log sigma^2 and
    by a factor e^36.4 (sixteen orders of magnitude) in the nugget"""
    return np.stack([theta(regime(n, kernel), True) for n in MIX_NAMES])


def mixture_weights(kind):
    S = len(MIX_NAMES)
    return np.ones(S) if kind == "uniform" else np.random.default_rng(ANALYSIS_SEED).dirichlet(np.ones(S))


@functools.lru_cache(maxsize=None)
def mixture_reference(kernel, wkind):
    """(float64 restatement, bars, disagreements) of marginal_restate.mixture on the `base` design and targets with caller weights, by the
    convention of test_gpu_marginal.py: the device is allowed 100 x the float64 / long double disagreement, floored at 2^-52, relative to
    max|mean|, max within and the largest d_s^2; a disagreement above 1e-8 is refused"""
    import marginal_restate as mr
    r = regime("base", kernel)
    args = (r.X, r.t, mixture_thetas(kernel), r.Xs, kernel, "zero", True, None, mixture_weights(wkind), None, True)
    a, b = mr.mixture(*args), mr.mixture(*args, dtype=LD)
    assert np.array_equal(a["ok"], b["ok"]) and a["ok"].all()
    scale = {"mean": float(np.abs(b["mean"]).max()), "within": float(b["within"].max()), "between": float(b["d2max"])}
    dis = {k: float(np.abs(a[k] - b[k]).max()) / sc for k, sc in scale.items()}
    bars = {k: MIX_MARGIN * max(dis[k], EPS) * scale[k] for k in scale}
    return a, bars, dis


@functools.lru_cache(maxsize=None)
def draw_normals(m=M):
    z = np.random.default_rng([ANALYSIS_SEED, m]).standard_normal((DRAWS, m))
    z.setflags(write=False)
    return z


def ladder_rung(cov, shift):
    """the rung of sample_restate's jitter ladder at which cov + shift I factorises in float64: 0 none needed, t >= 1 the t-th, -1 none does"""
    import sample_restate as sr
    dbar = float(np.mean(np.diag(cov)))
    for t, delta in enumerate([0.] + [sr.ladder_delta(k, dbar) for k in range(sr.LADDER_RUNGS)]):
        try:
            np.linalg.cholesky(cov + (shift + delta) * np.eye(cov.shape[0]))
            return t
        except np.linalg.LinAlgError:
            pass
    return -1


# ---- the variance bound -------------------------------------------------------------------------------------------------------------------------
VAR_RANKS = (32, 130)


@functools.lru_cache(maxsize=None)
def bound_inputs(name, kernel, Dn=D):
    """(K (N, N) without the nugget, cross covariances of the 37 queries (N, 37), K from long double rounded once) in float64"""
    import iterative_restate as ir
    r = regime(name, kernel, Dn)
    s, s2 = scales(r), sigma2(r)
    K, ks = ir.covariance(r.X, r.X, s, kernel, s2), ir.covariance(r.X, r.Xs, s, kernel, s2)
    K2 = np.asarray(ir.covariance(r.X, r.X, s, kernel, s2, dtype=LD), dtype=np.float64)
    for a in (K, ks, K2):
        a.setflags(write=False)
    return K, ks, K2


OWN_TRIALS = 6                                        # evaluations of K moved by an ulp per entry, next to the one rounded from long double


@functools.lru_cache(maxsize=None)
def bound_cache(name, kernel, Dn, rank, pivots=None):
    """(variance_bound_restate.cache on the given pivots (a tuple; None: its own), bar, cond(H), amp, own, first): the bar of
    test_gpu_variance_bound.py -- BARS["var"] at the scale of the prior variance sigma^2 + eta the bound is a difference from, amplified by
    cond(H) --; own: per column of R the LARGEST excess over the "fullcov" bar of the restatement on the same pivots of K rounded another
    way -- K from long double rounded once, and OWN_TRIALS copies of K with every entry moved one ulp up or down (symmetrically, seeded) --;
    first: the index of the first column with own > 1 (var_rank if none).  A column above 1 is not determined by float64 arithmetic:
    where the first prefix runs towards its cut by tau the pivots fall to 1e-10 of the first and a column is what is left of a column of L
    after the ones before it are projected out.  Column j of R combines the columns <= j of the factor, so the columns before `first` are
    held one by one and the ones behind it by R^T A R = I and the two-sided bound alone."""
    import variance_bound_restate as vr
    r = regime(name, kernel, Dn)
    K, ks, K2 = bound_inputs(name, kernel, Dn)
    ch = vr.cache(K, r.nugget, rank, pivots=pivots)
    rtol, atol = dc.BARS["var"]
    cond, amp = dc.amplification(ch.H)
    rng = np.random.default_rng([ANALYSIS_SEED, rank])
    own = np.zeros(ch.var_rank)
    for t in range(OWN_TRIALS + 1):
        Kp = K2
        if t:
            up = np.triu(rng.random(K.shape) < 0.5)
            up = up | up.T
            Kp = np.where(up, np.nextafter(K, np.inf), np.nextafter(K, -np.inf))
        other = vr.cache(Kp, r.nugget, ch.L.shape[1], pivots=ch.pivots)
        k = min(ch.var_rank, other.var_rank)
        own[k:] = np.inf
        own[:k] = np.maximum(own[:k], [dc.excess("fullcov", other.R[:, j], ch.R[:, j], amp) for j in range(k)])
    first = int(np.argmax(own > 1.)) if np.any(own > 1.) else ch.var_rank
    return ch, amp * (atol + rtol * (sigma2(r) + r.nugget)), cond, amp, own, first
