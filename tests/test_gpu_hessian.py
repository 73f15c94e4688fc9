"""Hessian of the log-posterior on the MI355X (mogp_emulator_amd.logpost_hessian / laplace_approximation, csrc/kernels_hess.hip) against
the NumPy restatement (hessian_restate.py), at the smallest shapes where the tiling can go wrong.

Tolerance.  Not fixed in advance: for every case the restatement is evaluated in float64 and in np.longdouble on the CPU, and the device
is allowed 100 x their disagreement relative to max|H| (its summation order and its exponential, <= 1.02 ulp, differ from NumPy's).  A case
whose float64 / long double disagreement exceeds 1e-8 would be too ill-conditioned to test a kernel with; every case asserts that it is
not.  Measured disagreements (this file prints them), hence bars: see DESIGN.md section 4.
"""
import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import _capi
from mogp_emulator_amd.GaussianProcessGPU import GPUUnavailableError
from mogp_emulator_amd.Laplace import LaplaceResult
from mogp_emulator_amd.Priors import GPPriors, InvGammaPrior, GammaPrior, LogNormalPrior, WeakPrior
from mogp_emulator_amd.libgpgpu import CorrTransform, CovTransform
from conftest import load_golden

import hessian_restate as hr

pytestmark = pytest.mark.gpu
MARGIN = 100.
ILL = 1e-8


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _data(n, D, seed=11):
    rng = np.random.default_rng(seed + 1000 * n + D)
    X = rng.random((n, D))
    t = np.sin(3 * X[:, 0]) + (X[:, 1] ** 2 if D > 1 else 0.) + .1 * rng.standard_normal(n)
    return X, t


def _theta(nc, D, fit, shift=0.):
    # correlation lengths of 0.1 - 0.6 times sqrt(D): the matrix stays well conditioned at every shape used here
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, nc) + shift if nc > 1 else np.array([np.log(1. / D) + 2.5 + shift])
    return np.concatenate([corr, [0.2 + shift], [-4.] if fit else []])


def _priors(nc, fit):
    fam = [InvGammaPrior(2.5, 0.7), WeakPrior(), LogNormalPrior(0.8, 1.3), GammaPrior(3., 0.4)]
    return GPPriors(corr=[fam[p % 4] for p in range(nc)], cov=GammaPrior(2., 1.5), nugget=InvGammaPrior(1.5, 1e-2) if fit else None,
                    nugget_type="fit" if fit else "fixed")


def _prior_d2(pri, theta, fit):
    nc = len(pri.corr)
    out = [p.d2logpdtheta2(float(np.exp(-0.5 * th)), CorrTransform()) for p, th in zip(pri.corr, theta)]
    out.append(pri.cov.d2logpdtheta2(float(np.exp(theta[nc])), CovTransform()))
    if fit:
        out.append(pri.nugget.d2logpdtheta2(float(np.exp(theta[nc + 1])), CovTransform()))
    return np.array(out)


def _reference(X, t, theta, kernel, fit, nugget, prior_d2, what):
    """float64 restatement and the device's bar: MARGIN x its disagreement with the long double restatement, relative to max|H|"""
    H = hr.hessian(X, t, theta, kernel, fit, nugget, prior_d2)
    HL = hr.hessian(X, t, theta, kernel, fit, nugget, prior_d2, dtype=np.longdouble)
    scale = float(np.abs(HL).max())
    dis = float(np.abs(H - HL).max()) / scale
    print("%s: float64 vs long double %.3g of max|H| = %.4g -> device bar %.3g" % (what, dis, scale, MARGIN * dis))
    assert dis <= ILL, "the case is too ill-conditioned to test a kernel with"
    return H, MARGIN * dis * scale


@functools.lru_cache(maxsize=None)
def _case(n, D, kernel, fit, golden=False):
    if golden:
        g = load_golden("c1_n200_d4.npz")
        X, t = g["X"], g["T"][0]
    else:
        X, t = _data(n, D)
    nc = 1 if kernel in hr.UNIFORM else D
    theta = _theta(nc, D, fit)
    pri = _priors(nc, fit)
    H, bar = _reference(X, t, theta, kernel, fit, None if fit else 1e-4, _prior_d2(pri, theta, fit), "n=%d D=%d %s %s" % (
        n, D, kernel, "fit" if fit else "fixed"))
    return X, t, theta, pri, H, bar


def _gp(X, t, kernel, fit, pri):
    return M.GaussianProcessGPU(X, t, kernel=kernel, nugget="fit" if fit else 1e-4, priors=pri)


def _close(got, want, bar, what):
    err = float(np.abs(got - want).max())
    print("%s: device vs float64 restatement %.3g (bar %.3g)" % (what, err, bar))
    assert np.all(np.isfinite(got))
    assert err <= bar, (what, err, bar)


SHAPES = [(33, 1, False), (33, 3, False), (130, 4, False), (200, 4, True), (257, 11, False)]


@pytest.mark.parametrize("fit", [True, False], ids=["fit", "fixed"])
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
@pytest.mark.parametrize("n,D,golden", SHAPES)
def test_device_matches_restatement(n, D, golden, kernel, fit):
    X, t, theta, pri, H, bar = _case(n, D, kernel, fit, golden)
    gp = _gp(X, t, kernel, fit, pri)
    got = M.logpost_hessian(gp, theta)
    assert got.shape == (theta.size, theta.size)
    assert np.array_equal(got, got.T)
    _close(got, H, bar, "n=%d D=%d %s" % (n, D, kernel))
    assert np.array_equal(M.logpost_hessian(gp, theta), got)           # two calls: the same bits


@pytest.mark.parametrize("kernel", ["UniformSqExp", "UniformMat52"])
def test_uniform_kernels(kernel):
    X, t, theta, pri, H, bar = _case(130, 4, kernel, True)
    got = M.logpost_hessian(_gp(X, t, kernel, True, pri), theta)
    assert got.shape == (3, 3) and np.array_equal(got, got.T)
    _close(got, H, bar, kernel)


def _live():
    c = ctypes.c_longlong(0)
    assert _capi.load().mogp_profile_counter(b"device_bytes_live", ctypes.byref(c)) == 0
    return c.value


def test_state_is_preserved():
    """log-posterior, gradient and predictions after a Hessian call (at the fitted theta, and at another one) are bit for bit what they
    were before it, and the device memory in use is back where it was"""
    X, t, theta, pri, H, bar = _case(130, 4, "Matern52", True)
    gp = _gp(X, t, "Matern52", True, pri)
    gp.fit(theta)
    Xs = np.random.default_rng(2).random((50, 4))

    def state():
        p = gp.predict(Xs)
        return gp.logposterior(theta), gp.logpost_deriv(theta), p.mean, p.unc, p.deriv
    before = state()
    live = _live()
    H0 = M.logpost_hessian(gp)                                         # theta=None: the fitted theta
    assert _live() == live
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    other = theta + 0.3
    H1 = M.logpost_hessian(gp, other)
    assert _live() == live
    assert not np.array_equal(H0, H1)
    th = gp.theta
    assert np.array_equal(np.concatenate([th.get_mean(), th.get_data()]), theta)
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    _close(H0, H, bar, "at the fitted theta")


def test_adaptive_nugget():
    """an adaptive nugget is the constant the device chose at the fit: a squared exponential with lengths of ~7 on 130 points in the unit
    cube needs a jitter (1.2e-6 on the host oracle)"""
    X, t = _data(130, 4)
    theta = np.array([-4., -4.5, -3.5, -4., 0.2])
    gp = M.GaussianProcessGPU(X, t, kernel="SquaredExponential", nugget="adaptive", priors=GPPriors(n_corr=4, nugget_type="adaptive"))
    gp.fit(theta)
    nug = gp.nugget
    got = M.logpost_hessian(gp)
    H = hr.hessian(X, t, theta, "SquaredExponential", False, nug)
    HL = hr.hessian(X, t, theta, "SquaredExponential", False, nug, dtype=np.longdouble)
    scale = float(np.abs(HL).max())
    dis = float(np.abs(H - HL).max()) / scale
    print("adaptive nugget %.3g: float64 vs long double %.3g" % (nug, dis))
    # the jitter is tiny by construction, so this case is ill-conditioned on purpose: it gets the bar its own disagreement gives
    _close(got, H, MARGIN * dis * scale, "adaptive")
    assert gp.nugget == nug


def _batch_model(kinds, devices=None):
    """emulators of one model with their own theta: every one uses the model's nugget type"""
    X, _ = _data(130, 4)
    rng = np.random.default_rng(9)
    T = np.array([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 + .1 * rng.standard_normal(130) for k in range(len(kinds))])
    return X, T


def test_batch_of_three_with_mixed_nugget_types_matches_single_calls():
    """three emulators of one model with different theta and nugget types fit / fixed / adaptive, in ONE call, against the same emulators one
    at a time: bit for bit"""
    X, T = _batch_model(range(3))
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget="fit", priors=GPPriors(n_corr=4, nugget_type="fit"))
    lib = mo._mogp_gpu
    lib.emulator(1).set_nugget_type(M.LibGPGPU.nugget_type(2))
    lib.emulator(1).set_nugget_size(1e-4)
    lib.emulator(2).set_nugget_type(M.LibGPGPU.nugget_type(0))
    widths = [lib.emulator(i).n_params() for i in range(3)]
    assert widths == [6, 5, 5]
    rows = np.zeros((3, 6))
    for i in range(3):
        rows[i, :widths[i]] = _theta(4, 4, widths[i] == 6, shift=0.1 * i)
    hess, ok = lib.hessian(rows)
    assert ok.all() and hess.shape == (3, 6, 6)
    for i in range(3):
        P = widths[i]
        single = lib.emulator(i).logpost_hessian(rows[i, :P])
        assert np.array_equal(hess[i, :P, :P], single)
        assert np.all(np.isnan(hess[i, P:, :])) and np.all(np.isnan(hess[i, :, P:]))
    X0, t0 = X, T[0]
    H, bar = _reference(X0, t0, rows[0], "Matern52", True, None, None, "batch emulator 0")
    _close(hess[0], H, bar, "batch emulator 0")


def test_batch_of_nine():
    """nine emulators: more batch slots than the eight the grid decode of the tile kernels packs together"""
    X, T = _batch_model(range(9))
    mo = M.MultiOutputGP_GPU(X, T, kernel="SquaredExponential", nugget=1e-4, priors=GPPriors(n_corr=4, nugget_type="fixed"))
    rows = np.array([_theta(4, 4, False, shift=0.05 * i) for i in range(9)])
    hess = M.logpost_hessian(mo, rows)
    assert hess.shape == (9, 5, 5) and hess.ok.all() and hess.fitted == list(range(9))
    for i in (0, 4, 8):
        assert np.array_equal(hess[i], mo._mogp_gpu.emulator(i).logpost_hessian(rows[i]))
    H, bar = _reference(X, T[8], rows[8], "SquaredExponential", False, 1e-4, None, "batch of nine, emulator 8")
    _close(np.asarray(hess[8]), H, bar, "batch of nine, emulator 8")


@pytest.mark.parametrize("devices", [None, "all"])
def test_multi_output(devices):
    if devices == "all" and M.LibGPGPU.device_count() < 2:
        pytest.skip("one device")
    X, T = _batch_model(range(4))
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget="fit", priors=GPPriors(n_corr=4, nugget_type="fit"), devices=devices)
    rows = np.array([_theta(4, 4, True, shift=0.1 * i) for i in range(4)])
    mo.fit_emulator(0, rows[0])
    mo.fit_emulator(2, rows[2])
    hess = M.logpost_hessian(mo)                                       # the fitted theta of emulators 0 and 2; 1 and 3 are not fit
    assert hess.shape == (4, 6, 6) and hess.fitted == [0, 2]
    assert np.all(np.isnan(hess[1])) and np.all(np.isnan(hess[3]))
    assert mo.get_indices_fit() == [0, 2]
    for i in (0, 2):
        assert np.array_equal(hess[i], M.logpost_hessian(mo.emulators[i], rows[i]))
    res = M.laplace_approximation(mo)
    assert res[1] is None and isinstance(res[0], LaplaceResult) and np.array_equal(res[2].hessian, hess[2])
    full = M.logpost_hessian(mo, rows)                                 # explicit rows: every emulator, fit or not (they are fit afterwards)
    assert np.array_equal(full[0], hess[0]) and np.array_equal(full[2], hess[2]) and np.all(np.isfinite(full))


def test_laplace_on_the_tsunami_fit():
    data, g = load_golden("tsunamidata.npz"), load_golden("tsunami_fit.npz")
    X, t, theta, nug = data["inputs"], data["targets"][0], g["theta"][0], float(g["nugget"][0])
    pri = GPPriors.default_priors(X, X.shape[1], "adaptive")
    gp = M.GaussianProcessGPU(X, t, nugget="adaptive", priors=pri)
    gp.fit(theta)
    nug = gp.nugget
    d2 = _prior_d2(pri, theta, False)
    H = hr.hessian(X, t, theta, "SquaredExponential", False, nug, d2)
    HL = hr.hessian(X, t, theta, "SquaredExponential", False, nug, d2, dtype=np.longdouble)
    scale = float(np.abs(HL).max())
    dis = float(np.abs(H - HL).max()) / scale
    print("tsunami: nugget %.3g, float64 vs long double %.3g of max|H| = %.4g" % (nug, dis, scale))
    assert dis <= ILL
    res = M.laplace_approximation(gp)
    _close(res.hessian, H, MARGIN * dis * scale, "tsunami")
    ev = np.linalg.eigvalsh(H)
    cond = float(np.abs(ev).max() / np.abs(ev).min())
    print("tsunami: eigenvalues %.4g .. %.4g, cond %.4g, is_minimum %s" % (ev[0], ev[-1], cond, res.is_minimum))
    # an eigenvalue moves by at most the norm of the perturbation (<= P x the entrywise bar)
    assert abs(ev[0]) > theta.size * MARGIN * dis * scale, "the sign of the smallest eigenvalue is not decided at this accuracy"
    assert res.is_minimum == bool(ev[0] > 0.)
    if res.is_minimum:
        want = np.sqrt(np.diag(np.linalg.inv(H)))
        assert_allclose(res.stderr, want, rtol=MARGIN * dis * cond, atol=0)
        assert res.sample(5, rng=0).shape == (5, theta.size)
    else:
        assert np.all(np.isnan(res.stderr)) and np.all(np.isnan(res.covariance))


def test_refusals():
    X, t = _data(33, 3)
    th = _theta(3, 3, False)
    gp = M.GaussianProcessGPU(X, t, nugget="pivot", priors=GPPriors(n_corr=3, nugget_type="pivot"))
    with pytest.raises(RuntimeError, match="pivot"):
        M.logpost_hessian(gp, th)
    gp = M.GaussianProcessGPU(X, t, kernel="ProductMat52", nugget=1e-4, priors=GPPriors(n_corr=3, nugget_type="fixed"))
    with pytest.raises(RuntimeError, match="ProductMat52"):
        M.logpost_hessian(gp, th)
    gp = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", nugget=1e-4)
    with pytest.raises(RuntimeError, match="mean function"):
        M.logpost_hessian(gp, np.concatenate([np.zeros(gp.n_params - th.size), th]))
    gp = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", nugget=1e-4, analytic_mean=True)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        M.logpost_hessian(gp, th)
    with pytest.raises(TypeError):
        M.logpost_hessian(object())


def test_reference_method_still_raises():
    X, t = _data(33, 3)
    gp = M.GaussianProcessGPU(X, t, nugget=1e-4)
    with pytest.raises(GPUUnavailableError):
        gp.logpost_hessian(_theta(3, 3, False))


def test_a_theta_that_cannot_be_factorised_fails_alone():
    """a fixed nugget of 0 with a length scale far beyond the design: every entry of the matrix is sigma^2 to rounding, which the host oracle
    cannot factorise either -- a refused input.  Its block is NaN with ok False; the other emulators of the batch are what they are alone."""
    from oracle import cpu_ref as R
    X, T = _batch_model(range(3))
    bad = np.array([-60., -60., -60., -60., 0.])
    with pytest.raises(Exception):
        R.GPRef(X, T[1], nugget=0.).fit(bad)
    mo = M.MultiOutputGP_GPU(X, T, nugget=0., priors=GPPriors(n_corr=4, nugget_type="fixed"))
    good = np.array([3., 3.5, 3., 3.5, 0.2])
    with pytest.raises(Exception):
        R.GPRef(X, T[0], nugget=0.).fit(bad)
    R.GPRef(X, T[0], nugget=0.).fit(good)
    hess, ok = mo._mogp_gpu.hessian(np.array([good, bad, good + 0.1]))
    assert list(ok) == [True, False, True]
    assert np.all(np.isnan(hess[1])) and np.all(np.isfinite(hess[0])) and np.all(np.isfinite(hess[2]))
    assert np.array_equal(hess[0], mo._mogp_gpu.emulator(0).logpost_hessian(good))
    with pytest.raises(RuntimeError, match="factorised"):
        mo._mogp_gpu.emulator(1).logpost_hessian(bad)
