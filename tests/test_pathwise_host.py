"""Host-side checks of the pathwise posterior draws (mogp_emulator_amd.IterativeGP.sample_paths): the plan and every refusal text of
csrc/predict_plan.h through a sanitised stand-alone program (tests/c/rff_plan_check.cpp), the argument refusals that need no device, and
the NumPy restatement (pathwise_restate.py) against itself:

* its float64 feature product lies inside the bar the device's product is held to (test_gpu_pathwise.py) against its long-double form, and a
  frequency matrix rounded to float32 misses it: the bar is not vacuous;
* the spectral measures: the feature kernel of the Philox streams lies within 6 sigma^2 / sqrt(F) of sigma^2 k (every term of the mean over
  f is bounded by 2 sigma^2 and the entry's standard deviation is at most sigma^2 / sqrt(F));
* the closed-form covariance of a path against the exact posterior covariance, printed (DESIGN.md section 3 records the figures).

PRODUCT_CASES, the inputs of the product and SEED are defined here and imported by test_gpu_pathwise.py."""
import importlib
import os

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

import dimension_cases as dc
import iterative_restate as ir
import pathwise_restate as pw
import test_iterative_host as th
from test_iterative_host import SIGMA2

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
# (M rows: 0 = the design's, else that many queries; N, D, F, S, kernel) of the feature product.  A pairwise-covering subset of
# M in {1, 63, 64, 65, 130} x F in {1, 3, 64, 65, 130, 256} x S in {1, 7, 16, 17, 33} x D in {1, 3, 17, 80}, with the design's rows and
# both query counts of dimension_cases (37, 65), a squared-exponential and a Matern kernel: every value occurs.
PRODUCT_CASES = [(0, 130, 3, 130, 33, "SquaredExponential"), (0, 130, 17, 65, 16, "Matern52"), (0, 130, 80, 256, 17, "Matern52"),
                 (0, 130, 1, 64, 7, "SquaredExponential"), (0, 64, 3, 3, 1, "Matern52"), (0, 63, 17, 1, 17, "SquaredExponential"),
                 (0, 65, 80, 130, 7, "SquaredExponential"), (0, 1, 3, 256, 16, "Matern52"),
                 (37, 130, 3, 256, 33, "Matern52"), (65, 130, 17, 130, 1, "SquaredExponential"), (37, 130, 80, 64, 33, "SquaredExponential"),
                 (65, 130, 1, 3, 16, "Matern52"), (1, 130, 17, 64, 17, "Matern52"), (63, 130, 1, 65, 33, "SquaredExponential"),
                 (64, 130, 80, 1, 7, "Matern52"), (65, 130, 3, 65, 7, "Matern52")]


def product_inputs(Mq, N, D, F, S, kernel):
    """(scaled points (M, D), scales, raw points or None for the design's rows, case, omega, phase, W (S, F))"""
    c, (s,) = th.setup(N, D, kernel, m=Mq if Mq else dc.M_TEST[0])
    omega, phase = pw.features(SEED, pw.STREAM, F, D, kernel)
    W = np.random.default_rng([SEED, F, S]).standard_normal((S, F))
    raw = c.Xs if Mq else None
    return ir.scaled(c.Xs if Mq else c.X, s), s, raw, c, omega, phase, W


def path_normals(n, S, F, seed=1):
    """the caller's normals of the GPU tests: (W (S, F), eps (S, n))"""
    rng = np.random.default_rng([seed, n, S, F])
    return rng.standard_normal((S, F)), rng.standard_normal((S, n))


def fraction_of_bar(got, truth80, bar):
    return float(np.max(np.abs(np.asarray(got.astype(np.longdouble) - truth80, dtype=np.float64)) / bar))


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
@pytest.mark.parametrize("Mq,N,D,F,S,kernel", PRODUCT_CASES, ids=lambda v: str(v))
def test_float64_product_lies_inside_the_bar_and_float32_frequencies_miss_it(Mq, N, D, F, S, kernel):
    Pt, s, raw, c, omega, phase, W = product_inputs(Mq, N, D, F, S, kernel)
    truth = pw.rff(Pt, omega, phase, W, SIGMA2, dtype=np.longdouble)
    bar = pw.rff_bar(Pt, omega, phase, W, SIGMA2)
    frac = fraction_of_bar(pw.rff(Pt, omega, phase, W, SIGMA2), truth, bar)
    rough = fraction_of_bar(pw.rff(Pt, omega.astype(np.float32).astype(np.float64), phase, W, SIGMA2), truth, bar)
    print("M %d D %d F %d S %d %s: float64 product at %.3g of the bar, float32 frequencies at %.3g" % (Pt.shape[0], D, F, S, kernel, frac, rough))
    assert truth.shape == (Pt.shape[0], S) and 0. < frac <= 1.
    assert rough > 1.


@pytest.mark.parametrize("kernel", th.FOUR)
@pytest.mark.parametrize("n,D", [(300, 3), (130, 1), (130, 17)])
def test_feature_kernel_lies_within_six_standard_deviations_of_the_kernel(n, D, kernel):
    c, (s,) = th.setup(n, D, kernel)
    Qt = ir.scaled(c.Xs, s)
    K = ir.covariance(c.Xs, c.Xs, s, kernel, SIGMA2)
    for F in (256, 1024, 4096):
        omega, phase = pw.features(0, pw.STREAM, F, D, kernel)
        worst = float(np.max(np.abs(pw.feature_kernel(Qt, Qt, omega, phase, SIGMA2) - K))) * np.sqrt(F) / SIGMA2
        print("n %d D %d %s F %d: feature kernel within %.3g sigma^2 / sqrt(F) of the kernel on the %d queries" % (n, D, kernel, F, worst, len(Qt)))
        assert worst <= 6.


@pytest.mark.parametrize("n,D,kernel", [(300, 3, "SquaredExponential"), (300, 3, "Matern52"), (130, 17, "SquaredExponential")])
def test_path_covariance_against_the_exact_posterior_covariance(n, D, kernel):
    c, (s,) = th.setup(n, D, kernel)
    omega, phase = pw.features(0, pw.STREAM, 4096, D, kernel)
    path, exact = pw.path_covariance(c.X, c.Xs, s, kernel, SIGMA2, dc.NUGGET, omega, phase)
    Qt = ir.scaled(c.Xs, s)
    prior = float(np.max(np.abs(pw.feature_kernel(Qt, Qt, omega, phase, SIGMA2) - ir.covariance(c.Xs, c.Xs, s, kernel, SIGMA2))))
    print("n %d D %d %s F 4096: posterior covariance error %.3g sigma^2, largest predictive variance %.3g sigma^2, prior covariance error %.3g sigma^2"
          % (n, D, kernel, np.max(np.abs(path - exact)) / SIGMA2, np.max(np.diag(exact)) / SIGMA2, prior / SIGMA2))
    assert np.all(np.isfinite(path)) and np.all(np.isfinite(exact))


def test_restatement_conditions_on_the_data():
    """f(X) + eta v + sqrt(eta) eps = y exactly in exact arithmetic: the dense-solve paths reproduce the targets to the solve's rounding"""
    n, D, kernel, S, F = 130, 3, "Matern52", 3, 64
    c, (s,) = th.setup(n, D, kernel)
    omega, phase = pw.features(SEED, pw.STREAM, F, D, kernel)
    rng = np.random.default_rng(5)
    W, eps = rng.standard_normal((S, F)), rng.standard_normal((S, n))
    f, v, b = pw.paths(c.X, c.T[0], c.X, s, kernel, SIGMA2, dc.NUGGET, omega, phase, W, eps)
    back = f + dc.NUGGET * v.T + np.sqrt(dc.NUGGET) * eps
    cond, amp = dc.amplification(ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET))
    assert np.max(np.abs(back - c.T[0][None, :])) <= cond * n * 2. ** -52 * np.max(np.abs(b))
    # antithetic normals average to the posterior mean
    f2 = pw.paths(c.X, c.T[0], c.Xs, s, kernel, SIGMA2, dc.NUGGET, omega, phase, np.vstack([W, -W]), np.vstack([eps, -eps]))[0]
    mean = ir.covariance(c.Xs, c.X, s, kernel, SIGMA2) @ np.linalg.solve(ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET), c.T[0])
    assert dc.excess("mean", 0.5 * (f2[:S] + f2[S:]), np.broadcast_to(mean, (S, len(mean))), amp) <= 1.


@pytest.mark.parametrize("n,D,kernel,p", th.PREDICT_SHAPES, ids=lambda v: str(v))
def test_restatement_converges_within_the_cap_on_the_right_hand_sides_of_the_paths(n, D, kernel, p):
    """what test_gpu_pathwise.py solves: y - g_s(X) - sqrt(eta) eps_s for the caller's normals of its tests (seeds 1 .. 4, F = 64)"""
    c, (s,) = th.setup(n, D, kernel)
    omega, phase = pw.features(0, pw.STREAM, 64, D, kernel)
    cols = []
    for seed, S in ((1, 3), (2, 1), (3, 3), (4, 2)):
        W, eps = path_normals(n, S, 64, seed=seed)
        cols.append(c.T[0][:, None] - pw.rff(ir.scaled(c.X, s), omega, phase, W, SIGMA2) - np.sqrt(dc.NUGGET) * eps.T)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    sv = ir.solve(K + dc.NUGGET * np.eye(n), np.column_stack(cols), ir.pivoted_cholesky(K, p)[0], dc.NUGGET, th.RTOL, th.MAX_ITER)
    print("n %d D %d %s p %d: at most %d iterations over the paths' right-hand sides" % (n, D, kernel, p, sv.iterations.max()))
    assert sv.converged.all() and sv.iterations.max() <= th.ITER_CAP


def test_restatement_converges_within_the_cap_on_the_right_hand_sides_of_the_large_design():
    """what test_gpu_pathwise_large.py solves: N = 1030, 130 features, 17 draws (seed 6)"""
    import large_design_cases as ld
    n, D, kernel, p = ld.ITER_SOLVE_SHAPES[0]
    c, (s,) = th.setup(n, D, kernel)
    omega, phase = pw.features(0, pw.STREAM, 130, D, kernel)
    W, eps = path_normals(n, 17, 130, seed=6)
    B = c.T[0][:, None] - pw.rff(ir.scaled(c.X, s), omega, phase, W, SIGMA2) - np.sqrt(dc.NUGGET) * eps.T
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    sv = ir.solve(K + dc.NUGGET * np.eye(n), B, ir.pivoted_cholesky(K, p)[0], dc.NUGGET, th.RTOL, th.MAX_ITER)
    print("n %d D %d %s p %d: at most %d iterations over the paths' right-hand sides" % (n, D, kernel, p, sv.iterations.max()))
    assert n == 1030 and sv.converged.all() and sv.iterations.max() <= th.ITER_CAP


def test_plan_memory_refusal_and_refusal_texts(tmp_path):
    out = th._build_and_run(tmp_path, "rff_plan_check")
    assert out.strip() == "ok 25 checks"


def test_exports():
    assert M.PosteriorPaths is IG.PosteriorPaths and M.path_features is IG.path_features
    assert hasattr(M.IterativeGP, "sample_paths") and hasattr(M.VecchiaGP, "sample_paths")
    for name in ("evaluate", "prior", "__call__"):
        assert hasattr(M.PosteriorPaths, name)
    om, ph = M.path_features(3, pw.STREAM + 8, 65, 4, 1)
    want = pw.features(3, pw.STREAM + 8, 65, 4, "Matern52")
    assert np.array_equal(om, want[0]) and np.array_equal(ph, want[1]) and np.all(np.abs(ph) <= np.pi)
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
        for name in ("mogp_local_rff", "mogp_local_sample_paths"):
            assert name in _capi.SIGNATURES and name + "(" in header
        for method in ("rff", "sample_paths"):
            assert hasattr(LibGPGPU.LocalGP_GPU, method)


class _NoDevice(object):
    """stands for the native handle; anything that would go to the device is an error"""
    calls = 0

    def _touch(self, *a, **k):
        _NoDevice.calls += 1
        raise AssertionError("the device must not be reached")

    kmatvec = precondition = solve = predict_exact = rff = sample_paths = _touch

    def close(self):
        pass


def test_refusals_come_before_any_device_call():
    good = [(0, np.ones(3), 1.1, 1e-4, None, np.zeros(0))]
    v = M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=4)
    who = "IterativeGP.sample_paths: "
    for S in (0, -1, 2.5):
        with pytest.raises(ValueError, match=who + "n_draws must be at least 1"):
            v.sample_paths(S)
    for F in (0, -3, 65537, 10.5):
        with pytest.raises(ValueError, match=who + "n_features must be between 1 and 65536"):
            v.sample_paths(2, n_features=F)
    for fd in (-1, 0.5, 2 ** 31):
        with pytest.raises(ValueError, match=who + "first_draw must not be negative"):
            v.sample_paths(2, first_draw=fd)
    for seed in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError, match=who + "seed must be an integer"):
            v.sample_paths(2, seed=seed)
    for stream in (-1, 2 ** 32, 2 ** 32 - 8, 0.5):
        with pytest.raises(ValueError, match=who + "stream must be an integer"):
            v.sample_paths(2, stream=stream)
    rng = np.random.default_rng(0)
    for bad in (np.zeros((2, 15)), np.zeros((3, 16)), np.zeros(16), np.zeros((2, 16, 1))):
        with pytest.raises(ValueError, match=who + r"feature_normals must have shape \(n_draws, n_features\) = \(2, 16\)"):
            v.sample_paths(2, n_features=16, feature_normals=bad)
    for bad in (np.zeros((2, 8)), np.zeros((1, 9)), np.zeros(9)):
        with pytest.raises(ValueError, match=who + r"noise_normals must have shape \(n_draws, N\) = \(2, 9\)"):
            v.sample_paths(2, n_features=16, noise_normals=bad)
    for val in (np.nan, np.inf):
        W, e = rng.standard_normal((2, 16)), rng.standard_normal((2, 9))
        W[1, 3], e[0, 8] = val, val
        with pytest.raises(ValueError, match=who + "feature_normals must be finite"):
            v.sample_paths(2, n_features=16, feature_normals=W)
        with pytest.raises(ValueError, match=who + "noise_normals must be finite"):
            v.sample_paths(2, n_features=16, noise_normals=e)
    for e in (-1, 1, 0.5):
        with pytest.raises(ValueError, match=who + "emulator must be between 0 and 0"):
            v.sample_paths(2, emulator=e)
    # the paths themselves
    paths = M.PosteriorPaths(v, good[0], n_draws=2, n_features=16, omega=np.zeros((16, 3)), phase=np.zeros(16), feature_normals=np.zeros((2, 16)),
                             update=np.zeros((9, 2)))
    for call in (paths.evaluate, paths.prior, paths):
        for bad in (np.zeros((4, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
            with pytest.raises(ValueError, match="testing must have shape"):
                call(bad)
        q = rng.random((4, 3))
        q[0, 0] = np.inf
        with pytest.raises(ValueError, match="testing must be finite"):
            call(q)
        with pytest.raises(ValueError, match="max_points must not be negative"):
            call(rng.random((4, 3)), max_points=-1)
    assert _NoDevice.calls == 0
    v.close()
    with pytest.raises(RuntimeError, match=who + "the handle has been closed"):
        v.sample_paths(2)
    for call in (paths.evaluate, paths.prior):
        with pytest.raises(RuntimeError, match="the handle has been closed"):
            call(rng.random((4, 3)))
    assert _NoDevice.calls == 0
