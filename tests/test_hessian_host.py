"""Host checks of the log-posterior Hessian: the NumPy restatement (tests/hessian_restate.py) against finite differences of the CPU oracle's
gradient, the prior term of csrc/hostmath.h against Priors.py, and LaplaceResult on hand-made Hessians.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hessian_restate as hr                                        # noqa: E402
from oracle import cpu_ref as R                                     # noqa: E402
from mogp_emulator_amd.Laplace import LaplaceResult                 # noqa: E402

ORACLE = {"SquaredExponential": R.SQEXP, "Matern52": R.MAT52, "UniformSqExp": R.UNISQEXP, "UniformMat52": R.UNIMAT52}


def _data(n=33, D=3, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.random((n, D))
    t = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + .1 * rng.standard_normal(n)
    return X, t


def _theta(kernel, D):
    corr = [0.3] if kernel in hr.UNIFORM else list(np.linspace(0.3, 1.1, D) * np.where(np.arange(D) % 2, -1., 1.))
    return np.array(corr + [0.2, -4.])


@pytest.mark.parametrize("kernel", sorted(ORACLE))
def test_restatement_matches_finite_differences(kernel):
    """central differences (h = 1e-5) of the oracle's analytic gradient, fitted nugget log eta = -4 (weak priors): 1e-7 of max|H|, 100 x the
    finite difference's own error measured at these shapes (8e-10 / 1.3e-9)"""
    X, t = _data()
    th = _theta(kernel, X.shape[1])
    H = hr.hessian(X, t, th, kernel, nugget_fit=True)
    gp = R.GPRef(X, t, kernel=ORACLE[kernel], nugget="fit")
    h = 1e-5
    F = np.zeros_like(H)
    for j in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        F[:, j] = (gp.logpost_deriv(tp) - gp.logpost_deriv(tm)) / (2 * h)
    err = np.abs(H - F).max() / np.abs(H).max()
    print(kernel, "finite-difference disagreement", err)
    assert err <= 1e-7
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("kernel,nugget", [("SquaredExponential", 1e-4), ("Matern52", 1e-4), ("UniformSqExp", 1e-4)])
def test_restatement_constant_nugget(kernel, nugget):
    """a fixed (or adaptive) nugget is a constant: the Hessian over [corr | cov] against the oracle's gradient with that nugget"""
    X, t = _data()
    th = _theta(kernel, X.shape[1])[:-1]
    H = hr.hessian(X, t, th, kernel, nugget_fit=False, nugget=nugget)
    gp = R.GPRef(X, t, kernel=ORACLE[kernel], nugget=nugget)
    h = 1e-5
    F = np.zeros_like(H)
    for j in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        F[:, j] = (gp.logpost_deriv(tp) - gp.logpost_deriv(tm)) / (2 * h)
    # nugget 1e-4 instead of e^-4: the matrix is ~200 x worse conditioned and so is the finite difference (5e-6 measured at 1e-6)
    assert np.abs(H - F).max() / np.abs(H).max() <= 1e-5
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("uni,per", [("UniformSqExp", "SquaredExponential"), ("UniformMat52", "Matern52")])
def test_uniform_is_block_sum_of_per_dimension(uni, per):
    X, t = _data()
    D = X.shape[1]
    Hu = hr.hessian(X, t, np.array([0.4, 0.2, -4.]), uni, nugget_fit=True)
    Hd = hr.hessian(X, t, np.array([0.4] * D + [0.2, -4.]), per, nugget_fit=True)
    assert_allclose(Hu, hr.uniform_from_per_dimension(Hd, D), rtol=0, atol=1e-11 * np.abs(Hu).max())


def test_long_double_restatement_close():
    X, t = _data()
    th = _theta("Matern52", 3)
    H = hr.hessian(X, t, th, "Matern52", nugget_fit=True)
    HL = hr.hessian(X, t, th, "Matern52", nugget_fit=True, dtype=np.longdouble)
    assert HL.dtype == np.longdouble
    assert float(np.abs(H - HL).max() / np.abs(HL).max()) < 1e-10


def test_hostmath_prior_second_derivative_matches_python(tmp_path):
    """Priors::d2logpdtheta2 (csrc/hostmath.h), compiled for the host, against Priors.py's d2logpdtheta2 for every family"""
    from mogp_emulator_amd.Priors import InvGammaPrior, GammaPrior, LogNormalPrior, WeakPrior
    from mogp_emulator_amd.libgpgpu import CorrTransform, CovTransform
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "prior_d2_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "prior_d2_check.cpp"), "-o", exe])
    code = {InvGammaPrior: 0, GammaPrior: 1, LogNormalPrior: 2}
    corr = [InvGammaPrior(2.5, 0.7), GammaPrior(3., 0.4), LogNormalPrior(0.8, 1.3), WeakPrior()]
    cov, nug = GammaPrior(2., 1.5), InvGammaPrior(1.5, 1e-2)
    theta = np.array([0.3, -0.8, 1.4, 0.1, 0.6, -4.])

    def spec(p):
        return "%d %.17g %.17g" % ((code[type(p)], p.shape, p.scale) if type(p) in code else (3, 0., 0.))
    for nug_type, nd in ((1, 6), (2, 5)):
        text = "%d %d\n%s\n%s\n" % (len(corr), nug_type, "\n".join(spec(p) for p in corr + [cov, nug]), " ".join("%.17g" % x for x in theta))
        got = np.array(subprocess.check_output([exe], input=text.encode()).decode().split(), dtype=float)
        want = [p.d2logpdtheta2(float(np.exp(-0.5 * th)), CorrTransform()) for p, th in zip(corr, theta)]
        want.append(cov.d2logpdtheta2(float(np.exp(theta[4])), CovTransform()))
        if nug_type == 1:
            want.append(nug.d2logpdtheta2(float(np.exp(theta[5])), CovTransform()))
        assert got.shape == (nd,)
        assert_allclose(got, want, rtol=1e-13, atol=0)
        assert got[3] == 0.


def test_laplace_result_positive_definite():
    H = np.array([[4., 1.], [1., 3.]])
    r = LaplaceResult([0.5, -1.], H)
    assert r.is_minimum
    assert_allclose(r.covariance, np.linalg.inv(H), rtol=1e-14)
    assert_allclose(r.stderr, np.sqrt(np.diag(np.linalg.inv(H))), rtol=1e-14)
    draws = r.sample(200000, rng=1)
    assert draws.shape == (200000, 2)
    assert_allclose(draws.mean(0), [0.5, -1.], atol=5e-3)
    assert_allclose(np.cov(draws.T), np.linalg.inv(H), atol=5e-3)
    assert np.array_equal(r.sample(3, rng=7), r.sample(3, rng=np.random.default_rng(7)))


def test_laplace_result_indefinite():
    r = LaplaceResult([0., 0.], np.array([[1., 2.], [2., 1.]]))
    assert not r.is_minimum
    assert_allclose(r.eigenvalues, [-1., 3.], atol=1e-14)
    assert np.all(np.isnan(r.covariance)) and np.all(np.isnan(r.stderr))
    with pytest.raises(ValueError):
        r.sample(1)
    with pytest.raises(ValueError):
        LaplaceResult([0., 0.], np.eye(3))
