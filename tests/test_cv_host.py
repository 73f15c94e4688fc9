"""Host-side checks of cross-validation at the fitted hyperparameters: the fast form the device computes against a brute-force refit
per fold, both in long double (cv_restate.py); kfold_labels; the argument refusals of cross_validate that need no device; cv_plan
(csrc/predict_plan.h) through a sanitised host program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, validation

import cv_restate as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.mark.parametrize("case", cr.TABLE, ids=lambda c: "n%d-D%d-%s-%s-%s" % (c[0], c[1], "loo" if c[2] is None else "k%d" % c[2], c[3], c[4]))
def test_fast_form_is_the_brute_force_refit_in_long_double(case):
    """Both are backward-stable long-double evaluations of one quantity: they may differ by 64 cond_2(Q) 2^-64, relative to the largest
    entry of each quantity.  Measured: 3 - 4 orders below that."""
    X, t, theta, labels, k, kw = cr.table_case(*case)
    Q, _, _ = cr.build(X, t, theta, **kw)
    cond = float(np.linalg.cond(Q))
    a = cr.fast(X, t, theta, labels, k, dtype=LD, **kw)
    b = cr.brute(X, t, theta, labels, k, dtype=LD, **kw)
    bar = 64. * cond * 2. ** -64
    for q, (dis, scale) in cr.disagreement(a, b).items():
        print("cond %.3g, %s: fast vs brute force in long double %.3g of %.4g (bar %.3g)" % (cond, q, dis, scale, bar))
        assert dis <= bar, (q, dis, bar)
    # the float64 fast form is as good as a float64 refit: the conditioning is not squared
    f64 = cr.disagreement(cr.fast(X, t, theta, labels, k, **kw), a)
    assert max(d for d, _ in f64.values()) <= 1e-8


def test_kfold_labels():
    for n, k in [(7, 2), (7, 7), (33, 3), (130, 5), (257, 2), (200, 10)]:
        lab = M.kfold_labels(n, k)
        assert np.array_equal(lab, np.arange(n) % k)
        for rng in (3, np.random.default_rng(3)):
            sh = M.kfold_labels(n, k, rng=rng)
            sizes = np.bincount(sh, minlength=k)
            assert sh.shape == (n,) and sizes.sum() == n and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1
            assert np.array_equal(np.sort(sh), np.sort(lab))
        assert np.array_equal(M.kfold_labels(n, k, rng=3), M.kfold_labels(n, k, rng=3))
    assert not np.array_equal(M.kfold_labels(130, 5, rng=3), M.kfold_labels(130, 5, rng=4))
    assert not np.array_equal(M.kfold_labels(130, 5, rng=3), M.kfold_labels(130, 5))
    for n, k in [(7, 1), (7, 8), (1, 2), (7, 0)]:
        with pytest.raises(ValueError):
            M.kfold_labels(n, k)


class _Native(object):
    "what cross_validate reads of the native object before it calls into the library"
    def __init__(self, n, fitted=True):
        self._n, self._fitted = n, fitted

    def n(self):
        return self._n

    def theta_fit_status(self):
        return self._fitted

    def targets(self):
        return np.zeros(self._n)

    def cross_validate(self, *a, **kw):
        raise AssertionError("the device must not be reached")


def _stub(n=10, nugget=2, fitted=True, analytic=False):
    gp = M.GaussianProcessGPU.__new__(M.GaussianProcessGPU)
    gp._densegp_gpu = _Native(n, fitted)
    gp._nugget_type = LibGPGPU.nugget_type(nugget)
    gp._analytic_mean = analytic
    return gp


def test_cross_validate_refusals_without_a_device():
    with pytest.raises(TypeError):
        M.cross_validate(object())
    gp = _stub()
    for kw in [dict(k=1), dict(k=11), dict(k=0), dict(max_slots=-1), dict(folds=np.zeros(9, dtype=int)), dict(folds=np.zeros((10, 1), dtype=int)),
               dict(folds=np.arange(10) % 2 * 1.0), dict(folds=np.arange(10) % 3 - 1), dict(folds=np.arange(10) % 3, k=2),
               dict(folds=np.zeros(10, dtype=int)), dict(folds=np.array([0, 2] * 5)), dict(folds=np.arange(10) % 2, k=3)]:
        with pytest.raises(ValueError):
            M.cross_validate(gp, **kw)
    with pytest.raises(RuntimeError, match="pivot"):
        M.cross_validate(_stub(nugget=3), k=2)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        M.cross_validate(_stub(analytic=True), k=2)
    with pytest.raises(RuntimeError, match="not been fit"):
        M.cross_validate(_stub(fitted=False))
    # what is valid gets as far as the library
    for kw in [dict(), dict(k=2), dict(k=10), dict(folds=np.arange(10) % 3), dict(k=3, rng=1)]:
        with pytest.raises(AssertionError, match="must not be reached"):
            M.cross_validate(gp, **kw)
    assert validation.cross_validate is M.cross_validate and M.CrossValidationResult is validation.CrossValidationResult


def test_result_object():
    t = np.array([[1., 2., 3., 4.]])
    r = M.CrossValidationResult(folds=np.arange(4) % 2, targets=t, mean=t + np.array([[.1, -.1, .2, -.2]]), unc=np.full((1, 4), .04),
                                mahalanobis=np.ones((1, 2)), log_score=np.array([[-1., -2.]]), ok=np.ones((1, 2), dtype=bool),
                                nugget=np.array([.05]), include_nugget=False)
    assert r.k == 2
    np.testing.assert_allclose(r.standard_errors, np.array([[.1, -.1, .2, -.2]]) / .3, rtol=1e-12)
    np.testing.assert_allclose(r.rmse, [np.sqrt(.025)], rtol=1e-12)
    np.testing.assert_allclose(r.total_log_score, [-3.])
    r.include_nugget = True
    np.testing.assert_allclose(r.standard_errors, np.array([[.1, -.1, .2, -.2]]) / .2, rtol=1e-12)


def test_cv_plan_properties(tmp_path):
    """tests/c/cv_plan_check.cpp sweeps (E, k, NPsub, device slots, max_slots) itself and exits non-zero at the first property that
    fails; built with the address and undefined-behaviour sanitisers"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cv_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "cv_plan_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
