"""The covariance paths on the MI355X across the hyperparameter range (regime_cases.py): the deep tail of the exponential, subnormal and
zero entries, its clamp, K ~ sigma^2 I, K ~ sigma^2 1 1^T + eta I, sigma^2 of e^+-18, nuggets from 1e-12 to 1e2, and a pair of design points
1e-9 apart -- on one design of 130 points (three tiles, the last partial), 37 queries.  The reference is always an np.longdouble
restatement; test_regime_cases_host.py shows on the CPU that every regime is well enough conditioned for the bars below to apply unchanged
(amplification 1) and that float64 itself lies far inside them.  Every figure is printed as a fraction of its bar (pytest -s).

Bars, and the file each comes from
  generated entries       derived here, below
  logpost, grad, mean,    dimension_cases.BARS (those of tests/tools/fuzz_parity.py) x dimension_cases.amplification, the gradient's absolute
  var, deriv, fullcov     part x max(1, max|g|): as test_gpu_dimension_sweep.py
  Hessian                 test_gpu_hessian.py: 100 x the float64 / long double disagreement of hessian_restate, relative to max|H|; a
                          disagreement below n 2^-52 counts as n 2^-52 (NumPy's blocked sums can sit far inside what a fixed-order float64
                          sum of n terms reaches); the tests print which regimes took that floor
  cross-validation        test_gpu_cv.py: 100 x the disagreement of cv_restate.fast, at least 2^-52, relative to the largest entry of each
                          quantity (needle's mean, identically 0, relative to max|t|: regime_cases.cv_disagreement)
  LocalGP.predict         test_gpu_local.py: BARS["mean"], BARS["var"] x the amplification of each query's own matrix, on the device's lists
  VecchiaGP               test_gpu_vecchia.py: BARS["logpost"] for the value, BARS["grad"] for the gradient, on the device's lists
  exact-likelihood forms  test_gpu_exact_lik.py: exact_lik_restate.forms_bar, on the device's own panels
  predict_exact mean      test_gpu_iterative.py: BARS["mean"] + |A^-1 k*| |y - A alpha| for the device's alpha

The bar of a generated entry sigma^2 k(r2), relative, per entry.  The reference is long double FROM THE SAME float64 numbers the device
starts from, so the only error in r2 is that of its accumulation.  The matrix-free operator (kgen_sweep) stages scaled coordinates
u = fl(x s): each difference u_i - u_j carries half an ulp, its square one ulp, and each of the D additions half an ulp more: (D / 2 + 1)
ulps.  cov_full_kernel, behind get_K_matrix, stages x unscaled and adds e_d (x_i - x_j)^2 with e_d = exp(theta_d) from the host: the
product e_d (x_i - x_j) costs half an ulp more, (D / 2 + 1.5) ulps, and its reference is formed from x and e_d.  Both are allowed
(D + 1) (for D >= 3 the slack also holds the 1.5 ulps the Matern's a = sqrt(5 r2) adds through its two roundings).  A relative error of r2 enters k multiplied by the gain
|d log k / d r2| r2: r2 / 2 for the squared exponential (|d log k / d r2| = 1/2), (5/6) r2 (1 + a) / (1 + a + a^2 / 3) for the Matern
(|d log k / d r2| <= 5/6).  On top: the exponential's 1.3 ulps (exp_dev.h), one ulp for the product with sigma^2 and the stored value, and
for the Matern 3 for the prefactor 1 + a + (5/3) r2 and its product with the exponential (regime_cases.FIXED_ULPS).  So
      |got - want| <= 2^-52 (FIXED_ULPS + (D + 1) gain) |want|
An entry whose exact value lies below the smallest normal double is allowed two steps of the subnormal grid ON TOP of this -- not
instead of it: at the top of the subnormal range the gain is 354, and the r2 term alone is 1.4e3 ulps of a value that has lost no bit yet
-- and must be finite and >= 0.  In `needle` the off-diagonal must be exact zeros and the diagonal sigma^2 (+ eta) to the bit."""

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.LocalGP import _KERNELS
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import exact_lik_restate as er
import local_restate as lr
import regime_cases as rc
import vecchia_restate as vr
from regime_cases import LD
from test_exact_lik_host import caller_probes

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", rc.cases(), ids=lambda c: "%s-%s-D%d" % c)
DENSE_CASES = pytest.mark.parametrize("case", rc.cases(rc.DENSE_KERNELS), ids=lambda c: "%s-%s-D%d" % c)
NUGGETS = pytest.mark.parametrize("fit", [False, True], ids=["fixed", "fit"])
SUB = 64                      # LocalGP takes its hyperparameters from an emulator fitted on the first rows only


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _gp(r, fit, rows=None):
    X, t = (r.X, r.t) if rows is None else (r.X[:rows], r.t[:rows])
    return M.GaussianProcessGPU(X, t, kernel=r.kernel, nugget="fit" if fit else r.nugget,
                                priors=GPPriors(n_corr=X.shape[1], nugget_type="fit" if fit else "fixed"))


def _frac(tag, got, want, amp=1., gscale=1.):
    """dimension_cases.excess against a long-double reference, the difference taken in long double; NaN (hence a failure) for a NaN"""
    rtol, atol = dc.BARS[tag]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == np.shape(want), (tag, got.shape, np.shape(want))
    return float(np.max(np.abs(got.astype(LD) - want) / (amp * (atol * gscale + rtol * np.abs(want)))))


def _report(what, fracs):
    print("regime %s: %s" % (what, ", ".join("%s %.3g" % kv for kv in fracs.items())), flush=True)
    bad = {k: v for k, v in fracs.items() if not v <= 1.}
    assert not bad, "%s: beyond the bar (fractions of it): %s" % (what, bad)


def _native(r):
    return LibGPGPU.LocalGP_GPU(r.X, r.t[None, :])


# ---- generated entries ---------------------------------------------------------------------------------------------------------------------
def _check_entries(r, got, U1, U2, what, diagonal=None, weights=None):
    """got against sigma^2 k in long double; diagonal: the value the diagonal of a square matrix must have to the bit"""
    D = U1.shape[1]
    k, gain = rc.entries(U1, U2, r.kernel, weights)
    want = LD(rc.sigma2(r)) * k
    assert np.all(np.isfinite(got)) and np.all(got >= 0.), what
    off = np.ones(got.shape, dtype=bool)
    if diagonal is not None:
        off = ~np.eye(got.shape[0], dtype=bool)
        assert np.all(np.diag(got) == diagonal), (what, "the diagonal is not %r to the bit" % diagonal)
    if r.name == "needle":
        assert np.all(got[off] == 0.), (what, "a needle's off-diagonal must be exact zeros", float(np.abs(got[off]).max()))
    sub = (want < LD(rc.TINY)) & off
    return rc.entry_excess(np.where(off, got, 0.), np.where(off, want, LD(0)), gain, r.kernel, D), int(np.sum(sub)), int(np.sum(sub & (got > 0.)))


@CASES
def test_generated_entries(case):
    """get_K_matrix (cov_build_kernel), the columns of the matrix-free operator (kgen_sweep, read through unit vectors: a sum of one product
    and zeros is the entry itself) and the rectangular product at 37 queries, entry by entry"""
    r = rc.regime(*case)
    s2, U, Us = rc.sigma2(r), rc.staged(r, r.X), rc.staged(r, r.Xs)
    gp = _gp(r, False)
    gp.fit(rc.theta(r, False))
    fk, nsub, npos = _check_entries(r, gp.get_K_matrix(), r.X, r.X, "get_K_matrix", diagonal=s2, weights=rc.weights_libm(r))
    kt, h = _KERNELS[r.kernel][0], _native(r)
    eye = np.eye(rc.N)
    A = h.kmatvec(kt, rc.scales(r), s2, r.nugget, eye)
    R = h.kmatvec(kt, rc.scales(r), s2, r.nugget, eye, queries=r.Xs)
    h.close()
    assert A.shape == (rc.N, rc.N) and R.shape == (rc.M, rc.N)
    fa = _check_entries(r, A, U, U, "kmatvec", diagonal=s2 + r.nugget)[0]
    fr = _check_entries(r, R, Us, U, "rectangular kmatvec")[0]
    print("%d entries of K below the smallest normal double, %d of them positive on the device" % (nsub, npos))
    if case[:2] == ("underflow", "SquaredExponential"):
        assert npos > 0                                            # gradual underflow: the subnormal results are there
    _report("%s %s D=%d entries" % case, {"get_K_matrix": fk, "operator columns": fa, "rectangular product": fr})


# ---- dense engine --------------------------------------------------------------------------------------------------------------------------
def _dense_fractions(ref, f, g, mean, var, deriv, cov, fit):
    want_g = ref["grad"] if fit else ref["grad"][:-1]
    amp = ref["amp"]
    out = {"logpost": _frac("logpost", f, ref["logpost"], amp), "grad": _frac("grad", g, want_g, amp, max(1., float(np.abs(g).max()))),
           "mean": _frac("mean", mean, ref["mean"], amp), "var": _frac("var", var, ref["var"], amp)}
    if deriv is not None:
        out["deriv"] = _frac("deriv", deriv, ref["deriv"], amp)
    if cov is not None:
        out["fullcov"] = _frac("fullcov", cov, ref["fullcov"], amp)
    return out


@NUGGETS
@DENSE_CASES
def test_dense_engine(case, fit):
    """logposterior, logpost_deriv and predict (mean, variance, input derivative, full covariance at the 37 queries) of one emulator"""
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    theta = rc.theta(r, fit)
    gp = _gp(r, fit)
    f, g = gp.logposterior(theta), gp.logpost_deriv(theta)
    p = gp.predict(r.Xs, deriv=True)
    cov = gp.predict(r.Xs, full_cov=True, deriv=False).unc
    got = (np.float64(f), g, p.mean, p.unc, p.deriv, cov)
    what = "%s %s D=%d dense %s" % (*case, "fit" if fit else "fixed")
    _report(what, _dense_fractions(ref, *got, fit))
    if r.name == "needle":
        _report(what + " against the closed form of K = sigma^2 I", _dense_fractions(dict(rc.needle_closed_form(r), amp=1.), *got, fit))


@pytest.mark.parametrize("kernel", rc.DENSE_KERNELS)
def test_one_batch_of_every_regime(kernel):
    """one MultiOutputGP_GPU whose emulators hold one regime each (every regime on the shared design: all but `twin`), the nugget a
    parameter: one launch carries K ~ I beside K ~ 1 1^T and sigma^2 sixteen orders apart; each emulator against its own reference"""
    names = [n for n in rc.NAMES if n != "twin"]
    regs = [rc.regime(n, kernel) for n in names]
    T, thetas = np.stack([r.t for r in regs]), np.stack([rc.theta(r, True) for r in regs])
    mo = M.MultiOutputGP_GPU(regs[0].X, T, kernel=kernel, nugget="fit", priors=GPPriors(n_corr=rc.D, nugget_type="fit"))
    f, g, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    mo.fit(thetas)
    mean, var, deriv = mo.predict(regs[0].Xs, deriv=True)
    cov = mo.predict(regs[0].Xs, full_cov=True, deriv=False)[1]
    fracs = {}
    for e, n in enumerate(names):
        for q, v in _dense_fractions(rc.dense_reference(n, kernel), f[e], g[e], mean[e], var[e], deriv[e], cov[e], True).items():
            fracs["%s %s" % (n, q)] = v
    _report("%s batch" % kernel, fracs)


# ---- Hessian and cross-validation ----------------------------------------------------------------------------------------------------------
@NUGGETS
@CASES
def test_hessian(case, fit):
    r, h = rc.regime(*case), rc.hessian_reference(*case, fit)
    theta = rc.theta(r, fit)
    got = M.logpost_hessian(_gp(r, fit), theta)
    assert got.shape == (theta.size, theta.size) and np.array_equal(got, got.T) and np.all(np.isfinite(got))
    err = float(np.abs(got.astype(LD) - h["HL"]).max())
    print("float64 vs long double %.3g of max|H| = %.4g%s" % (h["dis"], h["scale"], ": below n 2^-52, the floor is the bar" if h["floored"] else ""))
    assert h["dis"] <= rc.ILL
    _report("%s %s D=%d hessian %s" % (*case, "fit" if fit else "fixed"), {"hessian": err / h["bar"]})


@pytest.mark.parametrize("k", [None, rc.CV_FOLDS], ids=["loo", "k5"])
@CASES
def test_cross_validation(case, k):
    r = rc.regime(*case)
    a, b = rc.cv_reference(*case, k)
    gp = _gp(r, False)
    gp.fit(rc.theta(r, False))
    res = M.cross_validate(gp) if k is None else M.cross_validate(gp, k=k)
    assert np.all(res.ok) and np.array_equal(res.folds, np.arange(rc.N) if k is None else np.arange(rc.N) % k)
    got = {"mean": res.mean, "var": res.unc, "mahalanobis": res.mahalanobis, "log_score": res.log_score}
    fracs = {}
    for q, (dis, scale) in rc.cv_disagreement(r, a, b).items():
        assert dis <= rc.ILL, (q, dis)
        assert np.all(np.isfinite(got[q]))
        fracs[q] = float(np.abs(got[q].astype(LD) - b[q]).max()) / (rc.CV_MARGIN * max(dis, rc.EPS) * scale)
    _report("%s %s D=%d cross-validation %s" % (*case, "loo" if k is None else "k=5"), fracs)


# ---- large-design paths --------------------------------------------------------------------------------------------------------------------
def _rows(tag, got, want, cond):
    return max(_frac(tag, got[j:j + 1], want[j:j + 1], max(1., float(cond[j]) * 1e-7)) for j in range(len(got)))


@CASES
def test_local_prediction(case):
    """LocalGP.predict at k = 30: the lists are the restatement's exactly, the values on them within the bars, refusals the restatement's"""
    r = rc.regime(*case)
    gp = _gp(r, False, rows=SUB)
    gp.fit(rc.theta(r, False))
    lg = M.LocalGP(gp, r.X, r.t, n_neighbours=rc.K_LOCAL)
    p = lg.predict(r.Xs, return_neighbours=True)
    lg.close()
    assert np.array_equal(p.neighbours, lr.neighbours(r.X, r.Xs, rc.scales(r), rc.K_LOCAL)[0])
    mean, var, ok, cond = rc.local_reference(r, p.neighbours)
    assert np.array_equal(p.ok, ok)
    _report("%s %s D=%d local" % case, {"mean": _rows("mean", p.mean[ok], mean[ok], cond[ok]), "var": _rows("var", p.unc[ok], var[ok], cond[ok])})


@CASES
def test_vecchia_value_and_gradient(case):
    """VecchiaGP at k = 30 in the identity order, the nugget a parameter"""
    r = rc.regime(*case)
    theta = rc.theta(r, True)
    vg = M.VecchiaGP(r.X, r.t, kernel=r.kernel, n_neighbours=rc.K_LOCAL, nugget="fit", order=np.arange(rc.N))
    vg.set_neighbours(theta=theta)
    nbr = vg.neighbours
    ll = vg.loglik(theta, grad=True)
    vg.close()
    assert np.array_equal(nbr, vr.ordered_neighbours(r.X, rc.scales(r), rc.K_LOCAL))
    terms, g, ok, cond = rc.vecchia_reference(r, nbr)
    assert np.array_equal(ll.ok, ok) and ok.all()
    amp = max(1., float(cond.max()) * 1e-7)
    _report("%s %s D=%d Vecchia" % case, {"value": _frac("logpost", np.float64(ll.value), terms.sum(), amp),
                                          "gradient": _frac("grad", ll.grad, g.sum(axis=0), amp, max(1., float(np.abs(ll.grad).max())))})


@CASES
def test_exact_likelihood_forms_and_exact_mean(case):
    """mogp_local_loglik_exact's quadratic forms on the device's own panels (15 probes, rank 32), and mogp_local_predict_exact's mean
    against the dense one; test_regime_cases_host.py shows that the restated solver converges in every regime at this rank and tolerance"""
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    kt, s, s2 = _KERNELS[r.kernel][0], rc.scales(r), rc.sigma2(r)
    h = _native(r)
    rank = h.precondition(kt, s, s2, r.nugget, rc.ITER_RANK)[0]
    g1, g2 = caller_probes(rc.N, rank, 15)
    pc = h.loglik_exact(0, kt, s, s2, r.nugget, rc.ITER_RANK, 1e-6, rc.ITER_MAX, g1, g2, grad=True, return_panels=True)
    mean, _, (its, conv, res), _, alpha = h.predict_exact(0, kt, s, s2, r.nugget, rc.ITER_RANK, rc.ITER_RTOL, rc.ITER_MAX, True, r.Xs,
                                                         return_alpha=True)
    h.close()
    assert pc["converged"].all() and conv and np.all(np.isfinite(pc["forms_data"])) and np.all(np.isfinite(pc["forms_probe"]))
    U, W = pc["x"], pc["w"]
    truth, bar = er.forms(r.X, s, r.kernel, s2, U, W), er.forms_bar(r.X, s, r.kernel, s2, U, W)
    probe = slice(1, U.shape[1])

    def worst(got, cols):
        b = bar[:, cols].sum(axis=1)
        e = np.abs(np.asarray(got.astype(LD) - truth[:, cols].sum(axis=1), dtype=np.float64))
        return float(np.max(np.where(e == 0., 0., e / np.where(b > 0., b, 1e-300))))
    fm = float(np.max(np.abs(mean.astype(LD) - ref["mean"]) / rc.exact_mean_bar(ref, r, alpha)))
    print("preconditioner rank %d, alpha in %d iterations, residual %.3g" % (rank, its, res))
    _report("%s %s D=%d iterative" % case, {"data forms": worst(pc["forms_data"], slice(0, 1)), "probe forms": worst(pc["forms_probe"], probe),
                                            "exact mean": fm})
