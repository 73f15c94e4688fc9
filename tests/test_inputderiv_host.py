"""Host-side checks of the input derivatives at large designs (mogp_emulator_amd.IterativeGP.matvec_inputderiv, predict(deriv=True),
PosteriorPaths.gradient): the plan and every refusal text of csrc/predict_plan.h through a sanitised stand-alone program
(tests/c/inputderiv_plan_check.cpp), the argument refusals that need no device, and the NumPy restatement (inputderiv_restate.py) against
itself, the oracle and a central difference:

* its float64 difference form lies inside the bar the device's sweep is held to (test_gpu_inputderiv.py) against its long-double form, and
  the expanded form q~_d sum g V - sum g x~_jd V misses that bar on every design away from the origin: the bar tells the two apart;
* its float64 feature derivative lies inside its bar, and a frequency matrix rounded to float32 misses it;
* the assembled gradient of a path equals a long-double central difference of pathwise_restate's own evaluation;
* the kernel derivative equals the oracle's kernel_inputderiv for the four kernels, on the points of the golden vectors.

SHIFTED_CASES, the inputs of the products and the fraction helpers are defined here and imported by test_gpu_inputderiv.py."""
import importlib
import os

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

import dimension_cases as dc
import inputderiv_restate as idr
import iterative_restate as ir
import pathwise_restate as pw
import test_iterative_host as th
import test_pathwise_host as ph
from test_iterative_host import SIGMA2

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
# (kernel, M queries, N, D, c columns, shift): every coordinate of the design and of the queries is moved by `shift`
SHIFTED_CASES = [("SquaredExponential", 70, 130, 3, 7, 0.), ("SquaredExponential", 70, 130, 3, 7, 100.), ("SquaredExponential", 37, 300, 17, 16, 1000.),
                 ("SquaredExponential", 65, 126, 1, 1, 1e4), ("Matern52", 70, 130, 3, 7, 100.), ("Matern52", 37, 300, 17, 16, 1000.),
                 ("Matern52", 65, 126, 1, 1, 1e4)]


def sweep_inputs(kernel, Mq, N, D, c, shift=0., seed=0):
    """(raw design, raw queries, scales, V (N, c), case): dimension_cases' points moved by `shift`"""
    cs, (s,) = th.setup(N, D, kernel, m=Mq)
    return cs.X + shift, cs.Xs + shift, s, th.matvec_input(N, c, seed=seed), cs


def fraction_of_bar(got, truth80, bar):
    """largest |got - truth| / bar over the entries whose bar is positive; an entry with a zero bar must be exact"""
    err = np.abs(np.asarray(np.asarray(got).astype(np.longdouble) - truth80, dtype=np.float64))
    assert not np.any(err[bar == 0.]), "an entry whose bar is zero is not exact"
    return float(np.max(err[bar > 0.] / bar[bar > 0.])) if np.any(bar > 0.) else 0.


@LONG
@pytest.mark.parametrize("kernel,Mq,N,D,c,shift", SHIFTED_CASES, ids=lambda v: str(v))
def test_float64_difference_form_lies_inside_the_bar_and_the_expanded_form_misses_it_off_the_origin(kernel, Mq, N, D, c, shift):
    X, Q, s, V, _ = sweep_inputs(kernel, Mq, N, D, c, shift)
    Qt, Xt = ir.scaled(Q, s), ir.scaled(X, s)
    truth = idr.kgrad_in(Qt, Xt, s, kernel, SIGMA2, V, dtype=np.longdouble)
    bar = idr.kgrad_bar(Qt, Xt, s, kernel, SIGMA2, V)
    frac = fraction_of_bar(idr.kgrad_in(Qt, Xt, s, kernel, SIGMA2, V), truth, bar)
    rough = fraction_of_bar(idr.kgrad_expanded(Qt, Xt, s, kernel, SIGMA2, V), truth, bar)
    print("%s M %d N %d D %d c %d shift %g: difference form at %.3g of the bar, expanded form at %.3g" % (kernel, Mq, N, D, c, shift, frac, rough))
    assert truth.shape == (Mq, D, c) and 0. < frac <= 1.
    if shift > 0.:
        assert rough > 1.


@LONG
@pytest.mark.parametrize("Mq,N,D,F,S,kernel", ph.PRODUCT_CASES, ids=lambda v: str(v))
def test_float64_feature_derivative_lies_inside_the_bar_and_float32_frequencies_miss_it(Mq, N, D, F, S, kernel):
    Pt, s, raw, c, omega, phase, W = ph.product_inputs(Mq, N, D, F, S, kernel)
    truth = idr.rff_grad(Pt, s, omega, phase, W, SIGMA2, dtype=np.longdouble)
    bar = idr.rffgrad_bar(Pt, s, omega, phase, W, SIGMA2)
    frac = fraction_of_bar(idr.rff_grad(Pt, s, omega, phase, W, SIGMA2), truth, bar)
    rough = fraction_of_bar(idr.rff_grad(Pt, s, omega.astype(np.float32).astype(np.float64), phase, W, SIGMA2), truth, bar)
    print("M %d D %d F %d S %d %s: float64 feature derivative at %.3g of the bar, float32 frequencies at %.3g" % (Pt.shape[0], D, F, S, kernel, frac, rough))
    assert truth.shape == (Pt.shape[0], D, S) and 0. < frac <= 1.
    assert rough > 1.


@LONG
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_path_gradient_equals_a_long_double_central_difference_of_the_path(kernel):
    """f_s(x) = amp sum_f W_sf cos(omega_f . x~ + b_f) + sigma^2 sum_j k(r2_j) v_js by pathwise_restate.rff and iterative_restate.covariance in
    long double, at the float64 points x +- h e_d with h ~ 1e-5 / s_d (a step of 1e-5 in the scaled coordinate).  Along one scaled
    coordinate |d^3 cos| <= |omega_fd|^3 and |d^3 k| <= 12 for both families (the radial third derivative is at most 1.4 for the squared
    exponential and 5 sqrt(5) / 3 * 0.8 = 3 for Matern-5/2, at most 5 sqrt(5) = 11.2 with the transverse terms), |d k| <= 1: with
    M3 = amp sum_f |W_sf| |omega_fd|^3 + 12 sigma^2 sum_j |v_js| and M1 the same with the first powers and 1, the central difference is off
    by at most s_d [h~^2 M3 / 6 + 2^-52 (|x~_d| + h~) M1 / h~]: the truncation, and the rounding of the two scaled points to float64."""
    n, D, S, F = 130, 3, 3, 64
    c, (s,) = th.setup(n, D, kernel)
    omega, phase = pw.features(ph.SEED, pw.STREAM, F, D, kernel)
    W, eps = ph.path_normals(n, S, F, seed=5)
    Q = c.Xs[:9]
    v = pw.paths(c.X, c.T[0], Q, s, kernel, SIGMA2, dc.NUGGET, omega, phase, W, eps)[1]          # (n, S): what a PosteriorPaths holds as update
    got = idr.path_gradient(c.X, Q, s, kernel, SIGMA2, omega, phase, W, v, dtype=np.longdouble)
    assert got.shape == (S, 9, D)

    def value(P):
        return (pw.rff(ir.scaled(P, s), omega, phase, W, SIGMA2, dtype=np.longdouble)
                + ir.covariance(P, c.X, s, kernel, SIGMA2, dtype=np.longdouble) @ v.astype(np.longdouble)).T

    amp = np.sqrt(2. * SIGMA2 / F)
    worst = 0.
    for d in range(D):
        hs = 1e-5
        Qp, Qm = Q.copy(), Q.copy()
        Qp[:, d] += hs / s[d]
        Qm[:, d] -= hs / s[d]
        step = (Qp[:, d].astype(np.longdouble) - Qm[:, d].astype(np.longdouble))[None, :]
        fd = (value(Qp) - value(Qm)) / step
        m3 = amp * (np.abs(W) @ np.abs(omega[:, d]) ** 3) + 12. * SIGMA2 * np.abs(v).sum(axis=0)
        m1 = amp * (np.abs(W) @ np.abs(omega[:, d])) + SIGMA2 * np.abs(v).sum(axis=0)
        bound = s[d] * (hs ** 2 * m3[:, None] / 6. + 2. ** -52 * (np.abs(ir.scaled(Q, s)[:, d])[None, :] + hs) * m1[:, None] / hs)
        err = np.abs(np.asarray(got[:, :, d] - fd, dtype=np.float64))
        worst = max(worst, float(np.max(err / bound)))
        assert np.max(np.abs(np.asarray(fd, dtype=np.float64))) > 1e3 * np.max(bound)        # the bound is small against what it bounds
    print("%s: path gradient within %.3g of the central difference's bound" % (kernel, worst))
    assert worst <= 1.
    # the float64 restatement agrees with its long-double form to the two bars
    f64 = idr.path_gradient(c.X, Q, s, kernel, SIGMA2, omega, phase, W, v)
    Qt, Xt = ir.scaled(Q, s), ir.scaled(c.X, s)
    bar = (np.transpose(idr.kgrad_bar(Qt, Xt, s, kernel, SIGMA2, v) + idr.rffgrad_bar(Qt, s, omega, phase, W, SIGMA2), (2, 0, 1))
           + 2. ** -52 * np.abs(f64))
    assert fraction_of_bar(f64, got, bar) <= 1.


@pytest.mark.parametrize("kernel", th.FOUR)
def test_kernel_derivative_is_the_oracles_kernel_inputderiv_on_the_golden_points(kernel):
    from conftest import load_golden
    from oracle import cpu_ref as R
    g = load_golden("kernels.npz")
    x1, x2 = g["x1"], g["x2"]
    corr = g["theta"][:dc.n_corr(kernel, x1.shape[1])]
    s = ir.scales(corr, x1.shape[1], kernel)
    # the restated kernel is the oracle's, and the oracle's is pinned to the golden vectors (test_oracle_golden.py; directly here where they exist)
    K = ir.covariance(x1, x2, s, kernel, 1.)
    np.testing.assert_allclose(K, R.kernel_f(x1, x2, corr, kernel), rtol=1e-13)
    if kernel + "_K" in g.files:
        np.testing.assert_allclose(K, g[kernel + "_K"], rtol=1e-13)
    want = R.kernel_inputderiv(x1, x2, corr, kernel)           # (D, n1, n2) d k(x1_i, x2_j) / d x1_id
    Qt, Xt = ir.scaled(x1, s), ir.scaled(x2, s)
    gen = idr.generated(Qt, Xt, kernel, 1.)
    for d in range(x1.shape[1]):
        np.testing.assert_allclose(2. * s[d] * gen * (Qt[:, d][:, None] - Xt[:, d][None, :]), want[d], rtol=1e-12, atol=1e-15)
    # and through the product: V = the identity's columns
    G = idr.kgrad_in(Qt, Xt, s, kernel, 1., np.eye(x2.shape[0]))
    np.testing.assert_allclose(np.transpose(G, (1, 0, 2)), want, rtol=1e-12, atol=1e-15)


def test_a_query_on_a_design_point_gets_an_exact_zero_from_it_in_the_restatement():
    for kernel in ("SquaredExponential", "Matern52"):
        x = np.array([[0.3, 0.7]])
        s = np.array([1.7, 0.4])
        G = idr.kgrad_in(ir.scaled(x, s), ir.scaled(x, s), s, kernel, SIGMA2, np.ones((1, 1)))
        assert G.shape == (1, 2, 1) and not G.any() and np.all(np.isfinite(G))


def test_plan_memory_refusal_and_refusal_texts(tmp_path):
    out = th._build_and_run(tmp_path, "inputderiv_plan_check")
    assert out.strip() == "ok 27 checks"


def test_exports():
    for name in ("gradient", "prior_gradient", "value_and_gradient"):
        assert hasattr(M.PosteriorPaths, name)
    assert hasattr(M.IterativeGP, "matvec_inputderiv")
    import inspect
    assert inspect.signature(M.IterativeGP.predict).parameters["deriv"].default is False
    assert inspect.signature(M.IterativePrediction.__init__).parameters["deriv"].default is None
    assert list(inspect.signature(M.IterativePrediction.__init__).parameters)[-1] == "deriv"
    assert M.IterativePrediction(1, None, True, 0., 1, None, None).deriv is None
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
        for name in ("mogp_local_kmatvec_inputderiv", "mogp_local_rff_inputderiv"):
            assert name in _capi.SIGNATURES and name + "(" in header
        for method in ("kmatvec_inputderiv", "rff_inputderiv"):
            assert hasattr(LibGPGPU.LocalGP_GPU, method)
    text = open(os.path.join(ROOT, "mogp_emulator_amd", "IterativeGP.py")).read()
    assert "input derivatives of a path" not in text


class _NoDevice(object):
    """stands for the native handle; anything that would go to the device is an error"""
    calls = 0

    def _touch(self, *a, **k):
        _NoDevice.calls += 1
        raise AssertionError("the device must not be reached")

    kmatvec = precondition = solve = predict_exact = rff = sample_paths = kmatvec_inputderiv = rff_inputderiv = _touch

    def close(self):
        pass


def test_refusals_come_before_any_device_call():
    good = [(0, np.ones(3), 1.1, 1e-4, None, np.zeros(0))]
    v = M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=4)
    rng = np.random.default_rng(0)
    q = rng.random((4, 3))
    who = "IterativeGP.matvec_inputderiv: "
    for bad in (np.zeros(8), np.zeros((8, 2)), np.zeros((9, 0)), np.zeros((9, 2, 1))):
        with pytest.raises(ValueError, match=who + "V must have shape"):
            v.matvec_inputderiv(bad, q)
    b = rng.random((9, 2))
    b[3, 1] = np.nan
    with pytest.raises(ValueError, match=who + "V must be finite"):
        v.matvec_inputderiv(b, q)
    with pytest.raises(ValueError, match=who + "emulator must be between 0 and 0"):
        v.matvec_inputderiv(rng.random(9), q, emulator=1)
    paths = M.PosteriorPaths(v, good[0], n_draws=2, n_features=16, omega=np.zeros((16, 3)), phase=np.zeros(16), feature_normals=np.zeros((2, 16)),
                             update=np.zeros((9, 2)))
    calls = [lambda t, **k: v.matvec_inputderiv(rng.random(9), t, **k), lambda t, **k: v.predict(t, deriv=True, **k), paths.gradient,
             paths.prior_gradient, paths.value_and_gradient]
    for call in calls:
        for bad in (np.zeros((4, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
            with pytest.raises(ValueError, match="testing must have shape"):
                call(bad)
        bq = rng.random((4, 3))
        bq[0, 0] = np.inf
        with pytest.raises(ValueError, match="testing must be finite"):
            call(bq)
        for mp in (-1, 2.5):
            with pytest.raises(ValueError, match="max_points must not be negative"):
                call(q, max_points=mp)
    assert _NoDevice.calls == 0
    v.close()
    with pytest.raises(RuntimeError, match=who + "the handle has been closed"):
        v.matvec_inputderiv(rng.random(9), q)
    with pytest.raises(RuntimeError, match="IterativeGP.predict: the handle has been closed"):
        v.predict(q, deriv=True)
    for name in ("gradient", "prior_gradient"):
        with pytest.raises(RuntimeError, match="PosteriorPaths.%s: the handle has been closed" % name):
            getattr(paths, name)(q)
    with pytest.raises(RuntimeError, match="the handle has been closed"):
        paths.value_and_gradient(q)
    assert _NoDevice.calls == 0
