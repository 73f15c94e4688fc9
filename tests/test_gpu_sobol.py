"""Sobol indices fused behind the batched prediction (mogp_emulator_amd.sobol_indices, csrc/kernels_sobol.hip) on the MI355X:
against the NumPy restatement (sobol_restate.py) fed with the device's own public predictions and with the oracle's, emulator
variance, bitwise repeatability, forced chunking, the design= path, a multi-part model and the refusals.

Tolerances.  A relative error delta in the means moves S and ST by at most about 10 delta F / sigma, F = max |f|, sigma = sqrt(V)
(the numerators move by <= 2 delta F sigma (1 + sqrt 2), V relatively by <= 4 delta F / sigma).  Every comparison asserts F / sigma <= 10
first.  Device predictions agree between calls / chunkings to rtol 1e-8 (the chunking test of test_gpu_parity.py), so indices from the
device's own predictions are compared at atol 1e-6; device and oracle means agree to rtol 1e-7 (the mean-parity tests), so indices
from the oracle's predictions are compared at atol 1e-5.  The summation error itself is <= N 2^-53, far below both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import _capi
from mogp_emulator_amd.ExperimentalDesign import LatinHypercubeDesign, MonteCarloDesign
from mogp_emulator_amd.Priors import GPPriors
from oracle import cpu_ref as R
from conftest import load_golden

from sobol_restate import all_points, sobol_restate, split_points

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUG = 1e-6


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _inputs():
    g = load_golden("c1_n200_d4.npz")
    return g["X"], g["T"], g


def _samples(N, D, seed=5):
    rs = np.random.RandomState(seed)
    return rs.uniform(0., 1., (N, D)), rs.uniform(0., 1., (N, D))


def _restate_from(predict_mean, A, B):
    """predict_mean(points) -> (..., m); the restatement of the analysis and F / sigma of those values"""
    N, D = A.shape
    f = np.asarray(predict_mean(all_points(A, B)))
    r = sobol_restate(*split_points(f, N, D))
    r["F_over_sigma"] = np.max(np.abs(f), axis=-1) / np.sqrt(r["variance"])
    return r


def _check(res, want, atol, what):
    print(what, "F/sigma", want["F_over_sigma"], "max |dS|", np.max(np.abs(res.first_order - want["first_order"])),
          "max |dST|", np.max(np.abs(res.total - want["total"])))
    assert np.all(want["F_over_sigma"] <= 10.), "the bound on the indices needs F / sigma <= 10"
    assert_allclose(res.first_order, want["first_order"], rtol=0, atol=atol)
    assert_allclose(res.total, want["total"], rtol=0, atol=atol)
    assert_allclose(res.mean, want["mean"], rtol=1e-6)
    assert_allclose(res.variance, want["variance"], rtol=1e-6)


def _single(kernel="SquaredExponential", nugget=NUG, mean=None, analytic=False, which=0):
    X, T, g = _inputs()
    D = X.shape[1]
    nc = 1 if kernel.startswith("Uniform") else D
    kw = dict(mean=mean, analytic_mean=analytic) if mean is not None else {}
    gp = M.GaussianProcessGPU(X, T[which], kernel=kernel, nugget=nugget,
                              priors=GPPriors(n_corr=nc, nugget_type=nugget if isinstance(nugget, str) else "fixed"), **kw)
    return gp, X, T[which], g


# ---- 1. against the device's own predictions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_single_gp_matches_the_restatement_of_its_own_predictions(kernel):
    gp, X, t, g = _single(kernel)
    gp.fit(g[kernel + "_fixed_theta"])
    A, B = _samples(1 << 14, 4)
    res = M.sobol_indices(gp, A=A, B=B)
    assert res.first_order.shape == (4,) and res.total.shape == (4,) and np.ndim(res.mean) == 0 and np.ndim(res.variance) == 0
    assert res.emulator_variance is None
    want = _restate_from(lambda P: gp.predict(P, unc=False, deriv=False).mean, A, B)
    _check(res, want, 1e-6, "own predictions, " + kernel)
    # the container: attribute, key and positional access
    assert res["total"] is res.total and res[0] is res.first_order and len(list(res)) == 5


def _mogp(devices=None, nugget=1e-4):
    """four emulators on the golden inputs: the two golden targets, a target of inputs 0 and 1 only, a smooth target of all four"""
    X, T, g = _inputs()
    two = np.sin(2. * np.pi * X[:, 0]) + 1.5 * (X[:, 1] - 0.5) ** 2 * 4.
    allf = np.cos(3. * X @ np.array([1., -0.7, 0.5, 0.3])) + X[:, 3]
    T4 = np.stack([T[0], T[1], two, allf])
    th = g["SquaredExponential_fixed_theta"]
    thetas = np.stack([th, th + 0.1, np.array([1.5, 1.5, -6., -6., 0.]), th - 0.2])
    kw = {} if devices is None else dict(devices=devices)
    mo = M.MultiOutputGP_GPU(X, T4, nugget=nugget, priors=GPPriors(n_corr=4, nugget_type="fixed"), **kw)
    return mo, X, T4, thetas


def test_multi_output_matches_the_restatement_of_its_own_predictions():
    mo, X, T4, thetas = _mogp()
    mo.fit(thetas)
    A, B = _samples(1 << 13, 4, seed=6)
    res = M.sobol_indices(mo, A=A, B=B)
    assert res.first_order.shape == (4, 4) and res.total.shape == (4, 4) and res.mean.shape == (4,) and res.variance.shape == (4,)
    want = _restate_from(lambda P: mo.predict(P, unc=False, deriv=False).mean, A, B)
    _check(res, want, 1e-6, "own predictions, multi-output")


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------
N_ORACLE = 1 << 12


@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52", "UniformSqExp"])
def test_single_gp_vs_oracle(kernel):
    gp, X, t, g = _single(kernel)
    theta = g[kernel + "_fixed_theta"] if kernel != "UniformSqExp" else np.array([0.8, 0.1])
    gp.fit(theta)
    ref = R.GPRef(X, t, kernel=kernel, nugget=NUG)
    ref.fit(theta)
    A, B = _samples(N_ORACLE, 4, seed=7)
    want = _restate_from(lambda P: ref.predict(P, unc=False)[0], A, B)
    _check(M.sobol_indices(gp, A=A, B=B), want, 1e-5, "oracle, " + kernel)


def test_parametric_polynomial_mean_vs_oracle():
    """mean parameters inside theta (the reference GPU semantics): the oracle is the zero-mean GP on t - m(X), plus m"""
    gp, X, t, g = _single("Matern52", mean="c+c*x[0]+c*x[1]^2")
    beta = np.array([0.3, -0.4, 0.6])
    theta = g["Matern52_fixed_theta"]
    gp.fit(np.concatenate([beta, theta]))

    def m(P):
        return beta[0] + beta[1] * P[:, 0] + beta[2] * P[:, 1] ** 2
    ref = R.GPRef(X, t - m(X), kernel="Matern52", nugget=NUG)
    ref.fit(theta)
    A, B = _samples(N_ORACLE, 4, seed=8)
    want = _restate_from(lambda P: ref.predict(P, unc=False)[0] + m(P), A, B)
    _check(M.sobol_indices(gp, A=A, B=B), want, 1e-5, "oracle, parametric mean")


def test_analytic_mean_vs_oracle():
    gp, X, t, g = _single("SquaredExponential", mean="c+c*x[0]", analytic=True)
    theta = g["SquaredExponential_fixed_theta"]
    gp.fit(theta)
    ref = R.GPRefMean(X, t, [(0, 1)], True, kernel="SquaredExponential", nugget=NUG)
    ref.fit(theta)
    A, B = _samples(N_ORACLE, 4, seed=9)
    want = _restate_from(lambda P: ref.predict(P, unc=False)[0], A, B)
    _check(M.sobol_indices(gp, A=A, B=B), want, 1e-5, "oracle, analytic mean")


def test_pivot_nugget_vs_oracle():
    gp, X, t, g = _single("Matern52", nugget="pivot")
    theta = np.array([3.5, 3.0, 3.2, 2.8, 0.1])
    gp.fit(theta)
    ref = R.GPRef(X, t, kernel="Matern52", nugget="pivot")
    ref.fit(theta)
    A, B = _samples(N_ORACLE, 4, seed=10)
    want = _restate_from(lambda P: ref.predict(P, unc=False)[0], A, B)
    _check(M.sobol_indices(gp, A=A, B=B), want, 1e-5, "oracle, pivot")


def test_multi_output_vs_oracle_with_a_target_of_two_inputs_only():
    mo, X, T4, thetas = _mogp()
    mo.fit(thetas)
    A, B = _samples(N_ORACLE, 4, seed=11)
    refs = []
    for k in range(4):
        ref = R.GPRef(X, T4[k], kernel="SquaredExponential", nugget=1e-4)
        ref.fit(thetas[k])
        refs.append(ref)
    want = _restate_from(lambda P: np.stack([ref.predict(P, unc=False)[0] for ref in refs]), A, B)
    # emulator 2's target depends on inputs 0 and 1 only: first on the oracle's values, then on the device's
    print("oracle ST of the two-input target", want["total"][2])
    assert np.all(want["total"][2][2:] < 0.05) and np.all(want["total"][2][:2] > 0.2)
    res = M.sobol_indices(mo, A=A, B=B)
    _check(res, want, 1e-5, "oracle, multi-output")
    assert np.all(res.total[2][2:] < 0.05)


# ---- 3. unc=True -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_nugget", [True, False])
def test_emulator_variance_is_the_mean_predictive_variance(include_nugget):
    A, B = _samples(3000, 4, seed=12)
    AB = np.concatenate([A, B])
    gp, X, t, g = _single("Matern52")
    gp.fit(g["Matern52_fixed_theta"])
    res = M.sobol_indices(gp, A=A, B=B, unc=True, include_nugget=include_nugget)
    want = np.mean(gp.predict(AB, unc=True, deriv=False, include_nugget=include_nugget).unc)
    print("single", res.emulator_variance, want)
    assert np.ndim(res.emulator_variance) == 0 and res.emulator_variance > 0.
    assert_allclose(res.emulator_variance, want, rtol=1e-8)
    assert np.array_equal(res.first_order, M.sobol_indices(gp, A=A, B=B).first_order)      # unc changes nothing else
    mo, X, T4, thetas = _mogp()
    mo.fit(thetas)
    res = M.sobol_indices(mo, A=A, B=B, unc=True, include_nugget=include_nugget)
    want = np.mean(mo.predict(AB, unc=True, deriv=False, include_nugget=include_nugget).unc, axis=1)
    print("multi", res.emulator_variance, want)
    assert_allclose(res.emulator_variance, want, rtol=1e-8)


def test_emulator_variance_with_an_analytic_mean():
    A, B = _samples(2000, 4, seed=13)
    gp, X, t, g = _single("SquaredExponential", mean="c+c*x[0]", analytic=True)
    gp.fit(g["SquaredExponential_fixed_theta"])
    res = M.sobol_indices(gp, A=A, B=B, unc=True)
    assert_allclose(res.emulator_variance, np.mean(gp.predict(np.concatenate([A, B]), unc=True, deriv=False).unc), rtol=1e-8)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits():
    mo, X, T4, thetas = _mogp()
    mo.fit(thetas)
    A, B = _samples(1 << 13, 4, seed=14)
    a = M.sobol_indices(mo, A=A, B=B, unc=True)
    mo.predict(A[:100])                                              # other work on the engine in between
    b = M.sobol_indices(mo, A=A, B=B, unc=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------------
_CHUNK_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import mogp_emulator_amd as M
import test_gpu_sobol as T
mo, X, T4, thetas = T._mogp()
mo.fit(thetas)
A, B = T._samples(1000, 4, seed=15)
r = M.sobol_indices(mo, A=A, B=B, unc=True)
out = {k: np.asarray(r[k]).tolist() for k in ("first_order", "total", "mean", "variance", "emulator_variance")}
out["F"] = np.max(np.abs(mo.predict(T.all_points(A, B), unc=False, deriv=False).mean), axis=1).tolist()
print("SOBOL-JSON", json.dumps(out))
"""


def _run_chunk_script(env):
    script = _CHUNK_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SOBOL-JSON" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return {k: np.array(v) for k, v in json.loads(out.stdout.split("SOBOL-JSON")[-1]).items()}


def test_forced_small_chunks_agree_with_one_chunk():
    """MOGP_KS_BUDGET_GB = 1e-5 (10 kB, read once per process): 128 base rows per chunk of pass 2 -- eight chunks of the 1000 rows, the
    last one short -- and 128-point chunks inside every prediction."""
    whole = _run_chunk_script({})
    small = _run_chunk_script({"MOGP_KS_BUDGET_GB": "1e-5"})
    print("chunking: max |dS|", np.max(np.abs(whole["first_order"] - small["first_order"])),
          "max |dST|", np.max(np.abs(whole["total"] - small["total"])))
    print("chunking: F/sigma", whole["F"] / np.sqrt(whole["variance"]))
    assert np.all(whole["F"] / np.sqrt(whole["variance"]) <= 10.)
    assert_allclose(small["first_order"], whole["first_order"], rtol=0, atol=1e-6)
    assert_allclose(small["total"], whole["total"], rtol=0, atol=1e-6)
    assert_allclose(small["mean"], whole["mean"], rtol=1e-6)
    assert_allclose(small["variance"], whole["variance"], rtol=1e-6)
    assert_allclose(small["emulator_variance"], whole["emulator_variance"], rtol=1e-6)


# ---- 6. design= ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [MonteCarloDesign, LatinHypercubeDesign])
def test_design_path_draws_a_then_b(cls):
    gp, X, t, g = _single("SquaredExponential")
    gp.fit(g["SquaredExponential_fixed_theta"])
    np.random.seed(321)
    res = M.sobol_indices(gp, design=cls(4), n_base=2048)
    np.random.seed(321)
    d = cls(4)
    A = d.sample(2048)
    B = d.sample(2048)
    want = M.sobol_indices(gp, A=A, B=B)
    for x, y in zip(res, want):
        assert np.array_equal(x, y)
    np.random.seed(321)
    again = M.sobol_indices(gp, design=cls(4), n_base=2048)
    assert np.array_equal(again.total, res.total)
    with pytest.raises(ValueError):
        M.sobol_indices(gp, design=cls(4), n_base=2048, A=A, B=B)
    with pytest.raises(ValueError):
        M.sobol_indices(gp, design=cls(3), n_base=2048)
    with pytest.raises(ValueError):
        M.sobol_indices(gp)


# ---- 7. multi-part ---------------------------------------------------------------------------------------------------------------------------
def test_two_parts_on_one_device_match_the_single_engine():
    """the tolerance of test_gpu_multidevice.py for predictions: equal means, variances to 1e-15 absolute"""
    A, B = _samples(4096, 4, seed=16)
    single, X, T4, thetas = _mogp()
    multi = _mogp(devices=[0, 0])[0]
    assert multi._mogp_gpu.n_parts() == 2
    single.fit(thetas)
    multi.fit(thetas)
    a = M.sobol_indices(single, A=A, B=B, unc=True)
    b = M.sobol_indices(multi, A=A, B=B, unc=True)
    for k in ("first_order", "total", "mean", "variance"):
        assert np.array_equal(a[k], b[k]), k
    assert_allclose(b.emulator_variance, a.emulator_variance, rtol=0, atol=1e-15)


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_message():
    gp, X, t, g = _single("SquaredExponential")
    A, B = _samples(64, 4, seed=17)
    with pytest.raises((ValueError, RuntimeError), match="fit"):
        M.sobol_indices(gp, A=A, B=B)                                          # not fit yet
    with pytest.raises(RuntimeError, match="fit"):
        gp._densegp_gpu.sobol(A, B)                                            # the same from the library itself
    gp.fit(g["SquaredExponential_fixed_theta"])
    with pytest.raises((ValueError, RuntimeError), match="columns"):
        M.sobol_indices(gp, A=A[:, :3], B=B[:, :3])
    with pytest.raises((ValueError, RuntimeError), match="two base samples"):
        M.sobol_indices(gp, A=A[:1], B=B[:1])
    bad = A.copy()
    bad[5, 2] = np.nan
    with pytest.raises((ValueError, RuntimeError), match="finite"):
        M.sobol_indices(gp, A=bad, B=B)
    # the library's own checks, below the Python layer's
    lib = _capi.load()
    S, ST, mu, va = np.zeros(4), np.zeros(4), np.zeros(1), np.zeros(1)
    dp = _capi.dptr
    for a_, b_, n_, d_, word in ((A, B, 1, 4, "two base samples"), (bad, B, 64, 4, "finite"), (A, B, 16, 3, "columns")):
        assert lib.mogp_densegp_sobol(gp._densegp_gpu._h, dp(a_), dp(b_), n_, d_, 0, 1, dp(S), dp(ST), dp(mu), dp(va), None) != 0
        assert word in _capi.last_error()
    with pytest.raises(TypeError):
        M.sobol_indices(object(), A=A, B=B)


def test_unfitted_emulators_raise_or_give_nan_rows():
    mo, X, T4, thetas = _mogp()
    A, B = _samples(512, 4, seed=18)
    with pytest.raises(ValueError, match="fit"):
        M.sobol_indices(mo, A=A, B=B)
    for k in (0, 2, 3):
        mo.fit_emulator(k, thetas[k])
    with pytest.raises(ValueError, match="fit"):
        M.sobol_indices(mo, A=A, B=B)
    res = M.sobol_indices(mo, A=A, B=B, unc=True, allow_not_fit=True)
    assert np.all(np.isnan(res.first_order[1])) and np.all(np.isnan(res.total[1]))
    assert np.isnan(res.mean[1]) and np.isnan(res.variance[1]) and np.isnan(res.emulator_variance[1])
    mo.fit(thetas)
    full = M.sobol_indices(mo, A=A, B=B, unc=True)
    for k in (0, 2, 3):
        assert_allclose(res.first_order[k], full.first_order[k], rtol=0, atol=1e-6)
        assert_allclose(res.total[k], full.total[k], rtol=0, atol=1e-6)
        assert_allclose(res.emulator_variance[k], full.emulator_variance[k], rtol=1e-6)


def test_a_constant_emulator_has_nan_indices_and_zero_variance():
    X, T, g = _inputs()
    T2 = np.stack([np.zeros(X.shape[0]), T[0]])                    # zero mean function, constant target 0: the emulator is 0 everywhere
    th = g["SquaredExponential_fixed_theta"]
    mo = M.MultiOutputGP_GPU(X, T2, nugget=NUG, priors=GPPriors(n_corr=4, nugget_type="fixed"))
    mo.fit(np.stack([th, th]))
    A, B = _samples(1024, 4, seed=19)
    res = M.sobol_indices(mo, A=A, B=B, unc=True)
    assert res.variance[0] == 0. and res.mean[0] == 0.
    assert np.all(np.isnan(res.first_order[0])) and np.all(np.isnan(res.total[0]))
    assert np.all(np.isfinite(res.first_order[1])) and np.all(np.isfinite(res.total[1])) and res.variance[1] > 0.
    assert np.isfinite(res.emulator_variance[0])
    gp = M.GaussianProcessGPU(X, np.zeros(X.shape[0]), nugget=NUG, priors=GPPriors(n_corr=4, nugget_type="fixed"))
    gp.fit(th)
    one = M.sobol_indices(gp, A=A, B=B)
    assert one.variance == 0. and np.all(np.isnan(one.first_order)) and np.all(np.isnan(one.total))
