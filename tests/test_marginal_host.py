"""Host-side checks of the mixture prediction over hyperparameter samples: the restatement the device tests compare against
(marginal_restate.py) in float64 against long double and against stored reference outputs, the weight / ESS function against its formula
written out in long double, LaplaceResult.logpdf against the closed form, mixture_plan (csrc/predict_plan.h) through a sanitised host
program, and the argument validation of predict_marginal that needs no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import Marginal
from mogp_emulator_amd.Laplace import LaplaceResult
from conftest import load_golden

import marginal_restate as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _data(n, D, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.random((n, D))
    t = np.sin(3 * X[:, 0]) + (X[:, 1] ** 2 if D > 1 else 0.) + .1 * rng.standard_normal(n)
    return X, t, rng.random((9, D))


@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52", "UniformSqExp", "UniformMat52"])
@pytest.mark.parametrize("mean", ["zero", ("fixed", 0.3), "const"])
@pytest.mark.parametrize("fit", [False, True])
def test_float64_against_long_double(kernel, mean, fit):
    X, t, Xs = _data(40, 3)
    nc = 1 if kernel in mr.UNIFORM else 3
    rng = np.random.default_rng(1)
    S = 4
    base = np.concatenate([[0.2] if mean == "const" else [], np.log(1. / 3) + np.linspace(1., 3., nc), [0.1], [-5.] if fit else []])
    thetas = base + 0.2 * rng.standard_normal((S, base.size))
    w = np.array([.1, .4, 0., .5])
    a = mr.mixture(X, t, thetas, Xs, kernel, mean, fit, 1e-5, weights=w)
    b = mr.mixture(X, t, thetas, Xs, kernel, mean, fit, 1e-5, weights=w, dtype=LD)
    assert a["ok"].all() and b["ok"].all()
    assert_allclose(a["mean"], b["mean"].astype(float), rtol=0, atol=1e-9 * float(np.abs(b["mean"]).max()))
    assert_allclose(a["within"], b["within"].astype(float), rtol=0, atol=1e-9 * float(b["within"].max()))
    assert_allclose(a["between"], b["between"].astype(float), rtol=0, atol=1e-9 * float(b["d2max"]))
    assert_allclose(a["F"], b["F"].astype(float), rtol=1e-9, atol=0)
    assert b["between"].max() > 0 and b["weights"][2] == 0


@pytest.mark.parametrize("tag", ["SquaredExponential_fit", "Matern52_fit", "Matern52_fixed"])
def test_restatement_against_stored_reference_outputs(tag):
    """one theta, the reference's own log-posterior, means and variances (tests/golden/c1_n200_d4.npz)"""
    g = load_golden("c1_n200_d4.npz")
    kernel, kind = tag.split("_")
    fit = kind == "fit"
    mu, var, F, eta = mr.sample(g["X"], g["T"][0], g[tag + "_theta"], g["Xs"], kernel, "zero", fit, float(g[tag + "_nugget"]))
    assert_allclose(F, float(g[tag + "_logpost"]), rtol=1e-9)
    assert_allclose(mu, g[tag + "_mean"], rtol=1e-6, atol=1e-7)
    assert_allclose(var, g[tag + "_var_nonug"], rtol=0, atol=1e-7)
    assert_allclose(eta, float(g[tag + "_nugget"]), rtol=1e-12)
    # one sample with weight 1 is that sample
    r = mr.mixture(g["X"], g["T"][0], g[tag + "_theta"][None], g["Xs"], kernel, "zero", fit, float(g[tag + "_nugget"]), weights=[1.])
    assert np.array_equal(r["mean"], mu) and np.array_equal(r["within"], np.maximum(var + eta, 0.)) and not r["between"].any()


def _weights_long_double(F, ok, log_q):
    F, q, ok = np.asarray(F, dtype=LD), np.asarray(log_q, dtype=LD), np.asarray(ok, dtype=bool)
    good = np.flatnonzero(ok)
    a = good[np.argmin(F[good])]
    w = np.zeros(F.size, dtype=LD)
    w[good] = np.exp(-(F[good] - F[a]) - (q[good] - q[a]))
    w /= w.sum()
    return w, 1 / np.sum(w * w)


def test_weights_against_the_formula_in_long_double():
    rng = np.random.default_rng(3)
    for S in (1, 5, 33):
        F = 100. + 3. * rng.standard_normal(S)
        q = -2. + rng.standard_normal(S)
        ok = rng.random(S) > 0.2
        ok[0] = True
        w, ess = M.mixture_weights(F, ok, log_q=q)
        wl, el = _weights_long_double(F, ok, q)
        assert_allclose(w, wl.astype(float), rtol=1e-13, atol=0)
        assert_allclose(ess, float(el), rtol=1e-13)
        assert abs(w.sum() - 1.) < 1e-14 and np.all(w[~ok] == 0.)
        wr = mr.weights_of(F, ok, log_q=q)
        assert_allclose(w, wr, rtol=1e-13, atol=0)


def test_weights_hand_cases():
    w, ess = M.mixture_weights([7., 7., 7., 7.], [1, 1, 1, 1], log_q=[.5, .5, .5, .5])
    assert np.array_equal(w, np.full(4, .25)) and ess == 4.
    w, ess = M.mixture_weights([0., 800., 900.], [1, 1, 1], log_q=[0., 0., 0.])       # one dominant sample
    assert np.array_equal(w, [1., 0., 0.]) and ess == 1.
    w, ess = M.mixture_weights([5., 1., 5.], [1, 0, 1], log_q=[0., 0., 0.])           # the failed sample is the best one: ignored
    assert np.array_equal(w, [.5, 0., .5]) and ess == 2.
    w, ess = M.mixture_weights([5., 1., 5.], [1, 0, 1], weights=[1., 5., 3.])
    assert np.array_equal(w, [.25, 0., .75])
    w, ess = M.mixture_weights([np.nan, np.nan], [0, 0], log_q=[0., 0.])
    assert np.all(np.isnan(w)) and np.isnan(ess)
    w, ess = M.mixture_weights([1., 2.], [1, 1], weights=[0., 0.])                     # weights that sum to 0
    assert np.all(np.isnan(w)) and np.isnan(ess)
    w, ess = M.mixture_weights([[1., 1.], [np.nan, 3.]], [[1, 1], [0, 1]], log_q=np.zeros((2, 2)))
    assert np.array_equal(w, [[.5, .5], [0., 1.]]) and np.array_equal(ess, [2., 1.])
    # log q is only defined up to a constant; a sample the proposal favours more than the posterior does is weighted down
    a, _ = M.mixture_weights([3., 4., 5.], [1, 1, 1], log_q=[0., 1., -1.])
    b, _ = M.mixture_weights([3., 4., 5.], [1, 1, 1], log_q=[10., 11., 9.])
    assert_allclose(a, b, rtol=1e-15)
    assert_allclose(a, np.exp([0., -2., -1.]) / np.exp([0., -2., -1.]).sum(), rtol=1e-15)
    with pytest.raises(ValueError):
        M.mixture_weights([1.], [1])
    with pytest.raises(ValueError):
        M.mixture_weights([1.], [1], log_q=[0.], weights=[1.])
    with pytest.raises(ValueError):
        M.mixture_weights([1., 2.], [1], log_q=[0., 0.])


def test_logpdf_closed_form():
    rng = np.random.default_rng(4)
    P = 4
    A = rng.standard_normal((P, P))
    H = A @ A.T + P * np.eye(P)
    theta = rng.standard_normal(P)
    res = LaplaceResult(theta, H)
    th = theta + rng.standard_normal((6, P))
    d = th - theta
    want = -0.5 * P * np.log(2 * np.pi) + 0.5 * np.log(np.linalg.det(H)) - 0.5 * np.einsum("sp,pq,sq->s", d, H, d)
    assert_allclose(res.logpdf(th), want, rtol=1e-12)
    assert_allclose(res.logpdf(th[2]), want[2], rtol=1e-12)
    # it is a density: the one-dimensional case integrates to 1
    r1 = LaplaceResult([0.5], [[4.]])
    x = np.linspace(-5, 6, 20001)
    assert_allclose(np.sum(np.exp(r1.logpdf(x[:, None]))) * (x[1] - x[0]), 1., rtol=1e-9)
    with pytest.raises(ValueError):
        res.logpdf(np.zeros((2, P + 1)))
    with pytest.raises(ValueError):
        LaplaceResult([0., 0.], [[1., 0.], [0., -1.]]).logpdf(np.zeros((1, 2)))


def test_predict_marginal_argument_validation_without_a_device():
    X = np.zeros((3, 2))
    with pytest.raises(ValueError, match="weights need thetas"):
        M.predict_marginal(object(), X, weights=[1.])
    with pytest.raises(ValueError, match="n_samples"):
        M.predict_marginal(object(), X, n_samples=0)
    with pytest.raises(ValueError, match="max_slots"):
        M.predict_marginal(object(), X, max_slots=-1)
    with pytest.raises(TypeError):
        M.predict_marginal(object(), X)
    # the caller's own samples
    th, w = Marginal._check_samples(np.zeros((5, 3)), None, (), 3)
    assert th.shape == (5, 3) and np.array_equal(w, np.ones(5))
    th, w = Marginal._check_samples(np.zeros((2, 5, 3)), np.ones((2, 5)), (2,), 3)
    assert w.shape == (2, 5)
    for bad_th, bad_w, lead in [(np.zeros((5, 4)), None, ()), (np.zeros((0, 3)), None, ()), (np.zeros(3), None, ()),
                                (np.full((5, 3), np.nan), None, ()), (np.zeros((5, 3)), np.ones(4), ()),
                                (np.zeros((5, 3)), -np.ones(5), ()), (np.zeros((5, 3)), np.full(5, np.inf), ()),
                                (np.zeros((5, 3)), None, (2,)), (np.zeros((3, 5, 3)), None, (2,))]:
        with pytest.raises(ValueError):
            Marginal._check_samples(bad_th, bad_w, lead, 3)


def test_mixture_plan_properties(tmp_path):
    """tests/c/mixture_plan_check.cpp sweeps (E, S, slots, m, caps) itself and exits non-zero at the first property that fails; built
    with the address and undefined-behaviour sanitisers"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mixture_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "mixture_plan_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases ok" in out.stdout
