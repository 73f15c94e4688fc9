"""Host-side checks of the iterative exact likelihood (IterativeGP.log_likelihood, VecchiaGP.loglik_exact / fit_exact): the NumPy restatement
(exact_lik_restate.py) against dense linear algebra and against itself, the refusals that need no device, the exports and the plan
(tests/c/iter_lik_plan_check.cpp, sanitised).

* the restated estimator with dense solves equals the forms z^T A^-1 dA P^-1 z and u^T log(P^-1/2 A P^-1/2) u written out with explicit
  inverses and an explicit matrix square root; its Lanczos quadrature from the restatement's PCG at rtol 1e-10 agrees with the dense value --
  the REFERENCE GAP that test_gpu_exact_lik.py measures again on the device's own factor and allows the device four times;
* with 31 probes of a fixed seed every trace term and the log-determinant lie within 4 of their own standard errors of the dense values;
* at N = 127 the dense value and gradient are vecchia_restate's at k = 126, where the Vecchia likelihood is the exact one;
* L-BFGS-B on the restated estimator with the probes of ``fit_exact``'s seed, from theta of the data-generating GP + 0.7, succeeds, raises the
  dense likelihood and brings the dense gradient's norm below a tenth (the GPU test runs the same problem on the device).

``caller_probes``, the seeds, ``fit_problem`` and ``check_fit`` are imported by test_gpu_exact_lik.py."""
import importlib
import os

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Sampling import philox_normals

import dimension_cases as dc
import exact_lik_restate as er
import iterative_restate as ir
import test_iterative_host as th
import vecchia_cases as vc
import vecchia_restate as vr

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")
VG = importlib.import_module("mogp_emulator_amd.Vecchia")
SIGMA2, RTOL, MAX_ITER = th.SIGMA2, th.RTOL, th.MAX_ITER
UNBIASED_SEED = 0          # chosen on the restatement (test_unbiased_on_a_fixed_seed) and kept
FIT_SEED = 0               # of fit_exact's probes in the fit tests, host and device


def caller_probes(N, r, T, seed=0):
    """the caller's normals of the estimator tests: (g1 (r, T), g2 (N, T))"""
    g = np.random.default_rng([seed, N, T])
    return g.standard_normal((r, T)), g.standard_normal((N, T))


def test_plan_and_refusal_texts(tmp_path):
    assert th._build_and_run(tmp_path, "iter_lik_plan_check").strip() == "ok 12 checks"


def test_exports():
    assert M.ExactLogLik is IG.ExactLogLik and M.ExactFit is VG.ExactFit
    assert hasattr(M.IterativeGP, "log_likelihood") and hasattr(M.VecchiaGP, "loglik_exact") and hasattr(M.VecchiaGP, "fit_exact")
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        header = open(os.path.join(th.ROOT, "include", "mogp_hip.h")).read()
        assert "mogp_local_loglik_exact" in _capi.SIGNATURES and "mogp_local_loglik_exact(" in header
        assert hasattr(LibGPGPU.LocalGP_GPU, "loglik_exact")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
class _NoDevice(th._NoDevice):
    loglik_exact = vecchia_loglik = vecchia_neighbours = th._NoDevice._touch


def test_refusals_come_before_any_device_call(monkeypatch):
    th._NoDevice.calls = 0
    v = M.IterativeGP._on_handle(_NoDevice(), [(0, np.ones(3), 1.1, 1e-4, None, np.zeros(0))], 3, 9, precond_rank=4)
    who = "IterativeGP.log_likelihood"
    for T in (0, 32, -1, 2.5):
        with pytest.raises(ValueError, match="%s: n_probes must be between 1 and 31" % who):
            v.log_likelihood(n_probes=T)
    for seed in (-1, 0.5):
        with pytest.raises(ValueError, match="seed must be a non-negative integer"):
            v.log_likelihood(seed=seed)
    for bad in (3, (np.zeros((4, 2)),), (np.zeros((4, 2)), np.zeros((8, 2))), (np.zeros((4, 3)), np.zeros((9, 2))), (np.zeros(4), np.zeros((9, 1))),
                (np.zeros((4, 2)), np.zeros((9, 2, 1)))):
        with pytest.raises(ValueError, match="probes must be a pair"):
            v.log_likelihood(probes=bad)
    with pytest.raises(ValueError, match="n_probes must be between 1 and 31"):
        v.log_likelihood(probes=(np.zeros((4, 32)), np.zeros((9, 32))))
    g = np.zeros((9, 2))
    g[3, 1] = np.inf
    with pytest.raises(ValueError, match="probes must be finite"):
        v.log_likelihood(probes=(np.zeros((4, 2)), g))
    with pytest.raises(ValueError, match="emulator must be between 0 and 0"):
        v.log_likelihood(emulator=1)
    monkeypatch.setattr(VG, "_create_native", lambda inputs, residuals, device: _NoDevice())
    rng = np.random.default_rng(0)
    for nugget, P in (("fit", 5), (1e-3, 4)):
        vg = M.VecchiaGP(rng.random((9, 3)), rng.random(9), n_neighbours=4, nugget=nugget)
        good = np.zeros(P)
        for call in (vg.loglik_exact, vg.fit_exact):
            with pytest.raises(ValueError, match="theta must have %d entries" % P):
                call(np.zeros(P + 1))
            with pytest.raises(ValueError, match="n_probes must be between 1 and 31"):
                call(good, n_probes=32, precond_rank=4)
            with pytest.raises(ValueError, match=r"precond_rank must be between 0 and min\(N, 1024\) = 9"):
                call(good, precond_rank=10)
            with pytest.raises(ValueError, match="rtol must lie between 0 and 1"):
                call(good, rtol=1., precond_rank=4)
            with pytest.raises(ValueError, match="max_iter must be at least 1"):
                call(good, max_iter=0, precond_rank=4)
        with pytest.raises(ValueError, match="probes must be finite"):
            vg.loglik_exact(good, probes=(np.zeros((4, 2)), g), precond_rank=4)
    with pytest.raises(ValueError, match="the nugget must be positive"):
        M.VecchiaGP(rng.random((9, 3)), rng.random(9), n_neighbours=4, nugget=0.).loglik_exact(np.zeros(4), precond_rank=4)
    assert th._NoDevice.calls == 0


# ---- the estimator against dense values ---------------------------------------------------------------------------------------------------
def _setup(n, D, kernel, p):
    c, (s,) = th.setup(n, D, kernel)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    L = ir.pivoted_cholesky(K, p)[0] if p else np.zeros((n, 0))
    return c, s, K + dc.NUGGET * np.eye(n), L


@pytest.mark.parametrize("kernel", th.FOUR)
def test_estimator_against_dense_values(kernel):
    n, D, p, T = 300, 3, 64, 4
    c, s, A, L = _setup(n, D, kernel, p)
    g1, g2 = caller_probes(n, L.shape[1], T)
    y = c.T[0]
    dense = er.estimator_dense(c.X, y, s, kernel, SIGMA2, dc.NUGGET, L, g1, g2)
    # written out: explicit inverses, an explicit symmetric square root of P, the logarithm by the eigenvalues of the symmetric matrix
    P = L @ L.T + dc.NUGGET * np.eye(n)
    Ainv, Pinv = np.linalg.inv(A), np.linalg.inv(P)
    lam, Q = np.linalg.eigh(P)
    Ph = (Q / np.sqrt(lam)) @ Q.T
    mu, V = np.linalg.eigh(Ph @ A @ Ph)
    logM = (V * np.log(mu)) @ V.T
    z = dense["z"]
    cond = np.linalg.cond(A)
    tol = cond * n * 2. ** -52                                   # what a dense solve with A is off by, relative to the size of its terms
    per = er.length_derivatives(c.X, s, kernel, SIGMA2)
    for t in range(T):
        zt = z[:, t]
        for d, dA in enumerate(per):
            want = zt @ Ainv @ dA @ Pinv @ zt
            scale = np.linalg.norm(Ainv @ zt) * np.linalg.norm(dA, 2) * np.linalg.norm(Pinv @ zt)
            assert abs(dense["forms_each"][t, d] - want) <= tol * scale
        u = Ph @ zt
        want = u @ logM @ u
        assert abs(dense["quad"][t] - want) <= tol * (u @ u) * np.abs(np.log(mu)).max()
    # the Lanczos quadrature of the PCG coefficients: the reference gap
    pcg = er.estimator_pcg(c.X, y, s, kernel, SIGMA2, dc.NUGGET, L, g1, g2, RTOL, MAX_ITER)
    assert pcg["converged"].all()
    scale = dense["rho"] * np.abs(np.log(mu)).max()            # |u^T log(M) u| <= |u|^2 max|log mu|, |u|^2 = rho
    gap = np.abs(pcg["quad"] - dense["quad"]) / scale
    fgap = np.abs(pcg["forms_each"] - dense["forms_each"]).max() / np.abs(dense["forms_each"]).max()
    print("%s: iterations %s, reference gap of rho e1^T log(T) e1 at most %.3g of rho max|log mu| (%.3g absolute), of the probe forms %.3g" %
          (kernel, pcg["iterations"].tolist(), gap.max(), np.abs(pcg["quad"] - dense["quad"]).max(), fgap))
    # Gauss quadrature with m nodes is exact for polynomials of degree 2 m - 1: it converges at twice the rate of the CG error, which at the
    # stop is rtol in the residual and at most cond(P^-1/2 A P^-1/2) rtol in the solution; the dense value itself is off by tol
    assert gap.max() <= mu[-1] / mu[0] * RTOL + tol
    assert np.array_equal(pcg["alpha"], ir.solve(A, y[:, None], L, dc.NUGGET, RTOL, MAX_ITER).x[:, 0])     # the logged PCG is the restatement's


def test_float64_forms_lie_inside_the_bar_and_are_not_exact():
    if np.finfo(np.longdouble).eps >= 2. ** -60:
        pytest.skip("long double is no wider than double here")
    for kernel in th.FOUR:
        c, (s,) = th.setup(130, 3, kernel)
        U, W = th.matvec_input(130, 16, seed=1), th.matvec_input(130, 16, seed=2)
        truth = er.forms(c.X, s, kernel, SIGMA2, U, W)
        got = er.forms(c.X, s, kernel, SIGMA2, U, W, dtype=np.float64)
        frac = float(np.max(np.abs(np.asarray(got.astype(np.longdouble) - truth, dtype=np.float64)) / er.forms_bar(c.X, s, kernel, SIGMA2, U, W)))
        print("%s: float64 forms at %.3g of the bar" % (kernel, frac))
        assert 0. < frac <= 1.


@pytest.mark.parametrize("kernel", ["SquaredExponential", "UniformMat52"])
def test_unbiased_on_a_fixed_seed(kernel):
    n, D, p, T = 300, 3, 64, 31
    c, s, A, L = _setup(n, D, kernel, p)
    g1, g2 = caller_probes(n, L.shape[1], T, seed=UNBIASED_SEED)
    est = er.assemble(er.estimator_pcg(c.X, c.T[0], s, kernel, SIGMA2, dc.NUGGET, L, g1, g2, RTOL, MAX_ITER), n, dc.NUGGET, kernel)
    want = er.dense_loglik(c.X, c.T[0], s, kernel, SIGMA2, dc.NUGGET)
    zs = np.concatenate([[(est["logdet"] - want["logdet"]) / est["logdet_se"]], (est["trace"] - want["traces"]) / est["trace_se"]])
    print("%s: log|A| %.6f +- %.3g against %.6f; z-scores of the log-determinant and the traces %s" %
          (kernel, est["logdet"], est["logdet_se"], want["logdet"], np.round(zs, 2).tolist()))
    assert np.all(np.abs(zs) <= 4.)
    assert np.allclose(est["data_forms"], want["data_forms"], rtol=1e-6, atol=0.)


def test_dense_likelihood_is_vecchias_at_k_equal_to_n_minus_1():
    N, D, k = vc.LIMIT
    for kernel, fit in (("SquaredExponential", True), ("UniformMat52", False)):
        c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, fit)
        nbr = vr.ordered_neighbours(c.X, s, k)
        v, g = vr.loglik(c.X, c.T[0], s, kernel, sigma2, nugget, nbr, grad=True, fit_nugget=fit)
        want = er.dense_loglik(c.X, c.T[0], s, kernel, sigma2, nugget, fit_nugget=fit)
        cond = np.linalg.cond(ir.operator(c.X, s, kernel, sigma2, nugget))
        tol = cond * N * 2. ** -52
        assert abs(v - want["value"]) <= tol * abs(want["value"])
        assert np.all(np.abs(g - want["grad"]) <= tol * (np.abs(want["data_forms"]) + np.abs(want["traces"])))


VECCHIA_SEED, VECCHIA_RANK = 0, 64     # of the device's Vecchia-identity test: its probes are philox_normals(VECCHIA_SEED, .)


def test_seed_of_the_devices_vecchia_identity_on_the_restatement():
    N, D, k = vc.LIMIT
    kernel, T = "SquaredExponential", 31
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, True)
    L = ir.pivoted_cholesky(ir.covariance(c.X, c.X, s, kernel, sigma2), VECCHIA_RANK)[0]
    g1 = philox_normals(VECCHIA_SEED, IG._PROBE_STREAM, T, L.shape[1]).T
    g2 = philox_normals(VECCHIA_SEED, IG._PROBE_STREAM + 1, T, N).T
    est = er.assemble(er.estimator_pcg(c.X, c.T[0], s, kernel, sigma2, nugget, L, g1, g2, RTOL, MAX_ITER), N, nugget, kernel)
    want = er.dense_loglik(c.X, c.T[0], s, kernel, sigma2, nugget)
    zs = np.concatenate([[(est["logdet"] - want["logdet"]) / est["logdet_se"]], (est["trace"] - want["traces"]) / est["trace_se"]])
    print("z-scores of the log-determinant and the traces %s" % np.round(zs, 2).tolist())
    assert np.all(np.abs(zs) <= 4.)


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------------
FIT_KERNEL, FIT_RANK, FIT_PROBES, FIT_RTOL = "SquaredExponential", 64, 15, 1e-8


def fit_problem():
    """(X (300, 2), y drawn from the GP of theta_true, theta_true, the start theta_true + 0.7); the nugget is fitted"""
    n, D = 300, 2
    X = np.random.default_rng([11, n, D]).random((n, D))
    theta = np.array([np.log(10.), np.log(20.), 0., np.log(1e-2)])
    s, sigma2, nugget = vr.unpack(theta, D, FIT_KERNEL, "fit")
    return X, vr.draw(X, s, FIT_KERNEL, sigma2, nugget, 5), theta, theta + 0.7


def dense_at(X, y, theta):
    s, sigma2, nugget = vr.unpack(theta, X.shape[1], FIT_KERNEL, "fit")
    return er.dense_loglik(X, y, s, FIT_KERNEL, sigma2, nugget)


def restated_objective(X, y):
    """theta -> (-value, -grad) of the restated estimator on the probes fit_exact(seed=FIT_SEED) draws"""
    n = X.shape[0]
    G1 = philox_normals(FIT_SEED, IG._PROBE_STREAM, FIT_PROBES, FIT_RANK).T
    g2 = philox_normals(FIT_SEED, IG._PROBE_STREAM + 1, FIT_PROBES, n).T

    def f(theta):
        s, sigma2, nugget = vr.unpack(theta, X.shape[1], FIT_KERNEL, "fit")
        L = ir.pivoted_cholesky(ir.covariance(X, X, s, FIT_KERNEL, sigma2), FIT_RANK)[0]
        pc = er.estimator_pcg(X, y, s, FIT_KERNEL, sigma2, nugget, L, G1[:L.shape[1]], g2, FIT_RTOL, MAX_ITER)
        assert pc["converged"].all()
        out = er.assemble(pc, n, nugget, FIT_KERNEL)
        return -out["value"], -out["grad"]
    return f


def check_fit(X, y, start, theta, success):
    a, b = dense_at(X, y, start), dense_at(X, y, theta)
    print("dense log-likelihood %.4f -> %.4f, dense gradient norm %.4g -> %.4g, theta %s" %
          (a["value"], b["value"], np.linalg.norm(a["grad"]), np.linalg.norm(b["grad"]), np.round(theta, 3).tolist()))
    assert success
    assert b["value"] > a["value"]
    assert np.linalg.norm(b["grad"]) < 0.1 * np.linalg.norm(a["grad"])


def test_fit_on_the_restated_estimator():
    from scipy.optimize import minimize
    X, y, theta_true, start = fit_problem()
    res = minimize(restated_objective(X, y), start, method="L-BFGS-B", jac=True, options=dict(gtol=1e-5 * X.shape[0], ftol=1e-13, maxiter=200))
    check_fit(X, y, start, res.x, res.success)
