"""GPU parity tests (run with -m gpu on an MI355X).  Every call goes through the C ABI
(libmogp_hip.so) via the host-side mirror of the reference interface and is compared with
  * the golden vectors produced by the real reference (tests/golden/*.npz),
  * the oracle (oracle/cpu_ref.py) on the same seeded inputs,
  * size-independent identities at the BASELINE sizes.
Stated fp64 tolerances: K rtol 1e-13; L, alpha rtol 1e-8 on well-conditioned
fixtures; logpost rtol 1e-10 (1e-9 where cond(K) > 1e8); gradient rtol 1e-7 / atol 1e-8;
predictive mean rtol 1e-7; variance atol 1e-7 * sigma^2 (the reference's own GPU-vs-CPU bar,
tests/test_GaussianProcess.py:1017-1018, 1113-1118)."""
import os
import pickle

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, _capi
from mogp_emulator_amd.Priors import GPPriors, InvGammaPrior
from oracle import cpu_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

KERNELS = ["SquaredExponential", "Matern52"]
MODES = {"fixed": 1.e-6, "fit": "fit", "adaptive": "adaptive"}


def weak(D, nugget):
    return GPPriors(n_corr=D, nugget_type=nugget if isinstance(nugget, str) else "fixed")


def make_gp(X, t, kern="SquaredExponential", nugget=1e-6, priors="weak", **kw):
    X = np.asarray(X)
    D = 1 if X.ndim == 1 else X.shape[1]
    pri = weak(D, nugget) if priors == "weak" else priors
    return M.GaussianProcessGPU(X, t, kernel=kern, nugget=nugget, priors=pri, **kw)


def synth(seed, n, d, n_out, m):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    T = np.empty((n_out, n))
    for k in range(n_out):
        w = rng.normal(size=d)
        T[k] = np.sin(2 * np.pi * X @ w / np.sqrt(d)) + 0.1 * (X ** 2) @ np.abs(w) + 0.01 * rng.normal(size=n)
    return X, T, rng.uniform(0, 1, (m, d))


def test_device_is_gfx950_and_library_is_native():
    assert LibGPGPU.gpu_usable()
    assert LibGPGPU.have_compatible_device()


# ------------------------------------------------------------------------------------------------
# golden vectors of the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", KERNELS)
def test_fixture_2x3_known_answers(kern):
    g = load_golden("fixture_2x3.npz")
    for name, theta in (("ones", np.ones(4)), ("zeros", np.zeros(4))):
        pre = "%s_%s_" % (kern, name)
        gp = make_gp(g["X"], g["t"], kern, 0.)
        gp.fit(theta)
        assert_allclose(gp.current_logpost, g[pre + "logpost"], rtol=1e-13)
        assert_allclose(gp.L, g[pre + "L"], rtol=1e-12, atol=1e-15)
        assert_allclose(gp.Kinv_t, g[pre + "alpha"], rtol=1e-12)
        assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-9, atol=1e-13)
        assert_allclose(gp.get_K_matrix(), g[pre + "K"], rtol=1e-14)
        mean, unc, deriv = gp.predict(g["Xs"])
        assert_allclose(mean, g[pre + "mean"], rtol=1e-12)
        assert_allclose(unc, g[pre + "var"], rtol=1e-12)
    # literals held by the reference's own tests
    if kern == "SquaredExponential":
        gp = make_gp(g["X"], g["t"], kern, 0.)
        assert_allclose(gp.logposterior(np.ones(4)), 6.516671478123768, rtol=1e-13)
        assert_allclose(gp.predict(np.array([2., 3., 4.]))[0], [0.03390252374096476], rtol=1e-12)


@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("mode", list(MODES))
def test_grid11_all_nugget_modes(kern, mode):
    g = load_golden("grid11.npz")
    pre = "%s_%s_" % (kern, mode)
    theta = g[pre + "theta"]
    gp = make_gp(g["X"], g["t"], kern, MODES[mode])
    gp.fit(theta)
    assert_allclose(gp.nugget, g[pre + "nugget"], rtol=1e-13, atol=0)      # incl. adaptive jitter 1.3533528323661265e-07
    assert_allclose(gp.current_logpost, g[pre + "logpost"], rtol=1e-9)
    assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-7, atol=1e-8)
    mean, unc, _ = gp.predict(g["Xs"])
    sig2 = np.exp(theta[2])
    assert_allclose(mean, g[pre + "mean"], rtol=1e-7, atol=1e-10)
    assert_allclose(unc, g[pre + "var"], atol=1e-7 * sig2)
    assert_allclose(gp.predict(g["Xs"], include_nugget=False)[1], g[pre + "var_nonug"], atol=1e-7 * sig2)


@pytest.mark.parametrize("tag", ["c1_n200_d4", "n500_d10"])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("mode", ["fixed", "fit", "adaptive"])
def test_medium_configs_vs_reference(tag, kern, mode):
    """`adaptive` is the reference's DEFAULT nugget mode (GaussianProcess.py:204; linalg/cholesky.py:234-281: plain dpotrf first, jitter
    only when it fails).  On these fixtures the real reference factors K with ZERO jitter (golden nugget 0.0; cond(K) up to 1.1e9 for
    c1 / SquaredExponential, the other three 1e4 ... 3e5): the device must make the same decision -- nugget exactly 0.0 -- and then
    agree at what a zero-nugget matrix allows (measured in round 6, `tools/adaptive_edge.py`: logpost 3.5e-10, alpha 1.5e-9, gradient
    1.1e-9, mean 6.9e-10 at cond 1.1e9; 1e-14 ... 1e-12 on the other three)."""
    g = load_golden(tag + ".npz")
    pre = "%s_%s_" % (kern, mode)
    theta = g[pre + "theta"]
    gp = make_gp(g["X"], g["T"][0], kern, MODES[mode])
    gp.fit(theta)
    if mode == "adaptive":
        assert g[pre + "nugget"] == 0.0 and gp.nugget == 0.0          # the jitter / no-jitter DECISION, exactly
    K = gp.get_K_matrix()
    assert_allclose(K.sum(), g[pre + "K_sum"], rtol=1e-13)
    assert_allclose(K[::37, ::41], g[pre + "K_rows"], rtol=1e-13)
    assert_allclose(np.diag(gp.L), g[pre + "L_diag"], rtol=1e-8)
    assert_allclose(gp.L[::37, ::41], g[pre + "L_rows"], rtol=1e-7, atol=1e-10)
    assert_allclose(gp.Kinv_t, g[pre + "alpha"], rtol=1e-6, atol=1e-6 * np.abs(g[pre + "alpha"]).max())
    assert_allclose(gp.current_logpost, g[pre + "logpost"], rtol=1e-9)
    assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-7, atol=1e-7)
    mean, unc, _ = gp.predict(g["Xs"])
    assert_allclose(mean, g[pre + "mean"], rtol=1e-7, atol=1e-8)
    assert_allclose(unc, g[pre + "var"], atol=1e-7)
    if mode == "adaptive":
        assert_allclose(gp.predict(g["Xs"], include_nugget=False)[1], g[pre + "var_nonug"], atol=1e-7)
        # the decision must not depend on the batch an emulator is factored in (one workgroup per CU / two per CU / groups of eight)
        for B in (3, 16):
            mo = M.MultiOutputGP_GPU(g["X"], np.tile(g["T"][0], (B, 1)), kernel=kern, nugget="adaptive", priors=weak(g["X"].shape[1], "adaptive"))
            mo.fit(np.tile(theta, (B, 1)))
            assert np.all(mo._nuggets() == 0.0)
            assert_allclose([e.current_logpost for e in mo.emulators], g[pre + "logpost"], rtol=1e-9)


def adaptive_sweep_case():
    """C1's inputs, SquaredExponential, sigma^2 = 1, one shared log inverse squared length scale swept from -0.5 (cond 3e13) to -3.0 (K
    indefinite in fp64) in steps of 1/8: the adaptive nugget's knife-edge (linalg/cholesky.py:234-281).  Every point is classified by the
    pivots of K's Cholesky factorisation in 80-bit long double (oracle/exact.py knife_edge_class): with tau = 8 max(n, 32) eps max K_ii,
    "definite" when no exact pivot is below tau, "indefinite" when the first one below it is <= -tau, "band" otherwise -- where two fp64
    factorisations with different summation orders may decide differently (the reference's LAPACK succeeds down to a smallest pivot of
    0.01 tau and fails from 0.005 tau on)."""
    g = load_golden("c1_n200_d4.npz")
    X, t = g["X"], g["T"][0]
    ths = np.arange(-0.5, -3.01, -0.125)
    thetas = np.stack([np.r_[np.full(4, th), 0.] for th in ths])
    return X, t, thetas


def adaptive_sweep_check(X, t, thetas, verbose=False):
    from oracle import exact
    n = X.shape[0]
    B = len(thetas)
    mo = M.MultiOutputGP_GPU(X, np.tile(t, (B, 1)), nugget="adaptive", priors=weak(X.shape[1], "adaptive"))
    f, _, ok = mo._mogp_gpu.eval(thetas, grad=False)
    assert ok.all()
    mo.fit(thetas)
    nug = mo._nuggets()
    stats = dict(definite=0, indefinite=0, band=0, band_agree=0)
    for k in range(B):
        ref = R.GPRef(X, t, nugget="adaptive")
        lp = ref.fit(thetas[k])
        K = ref.get_K_matrix()
        cls, dmin = exact.knife_edge_class(K)
        rung0 = 1e-6 * K.diagonal().mean()
        ladder = [0.0] + [rung0 * 10. ** j for j in range(5)]
        solo = make_gp(X, t, nugget="adaptive"); solo.fit(thetas[k])
        if verbose:
            print("theta %.3f  %-10s pivot %9.4f tau  oracle nugget %g  device nugget %g (alone %g)  logpost oracle %.9g device %.9g" %
                  (thetas[k][0], cls, dmin, ref.nugget, nug[k], solo.nugget, lp, f[k]), flush=True)
        assert solo.nugget == nug[k], "the decision depends on the batch"            # and with it everything else
        assert solo.current_logpost == mo.emulators[k].current_logpost or not (os.environ.get("MOGP_CHOL"))
        assert any(abs(nug[k] - r) <= 1e-13 * r for r in ladder), (nug[k], ladder)   # zero or a rung of the reference's ladder
        if cls == "definite":
            stats["definite"] += 1
            assert ref.nugget == 0.0 and nug[k] == 0.0, (thetas[k][0], dmin, ref.nugget, nug[k])
            w = np.linalg.eigvalsh(K)
            condeps = float(w[-1] / w[0]) * 2. ** -52 if w[0] > 0. else np.inf      # (eigvalsh itself is off by ~ n eps |K| at the small end)
            if dmin >= 100. and condeps < 1e-2:
                assert_allclose(f[k], lp, rtol=max(1e-10, 0.05 * condeps))
        elif cls == "indefinite":
            stats["indefinite"] += 1
            assert ref.nugget > 0. and abs(nug[k] - ref.nugget) <= 1e-13 * ref.nugget, (thetas[k][0], dmin, ref.nugget, nug[k])
            assert_allclose(f[k], lp, rtol=1e-5)
        else:
            stats["band"] += 1
            if nug[k] > 0. and abs(nug[k] - ref.nugget) <= 1e-13 * ref.nugget:
                stats["band_agree"] += 1
                assert_allclose(f[k], lp, rtol=1e-5)      # K + 1e-6 I: cond ~ 1e8
            elif nug[k] == 0. and ref.nugget == 0.:
                stats["band_agree"] += 1                   # both factored a matrix with cond ~ 1 / eps: the values are rounding noise
            assert np.isfinite(f[k])
    return stats


def test_adaptive_nugget_decision_sweep_across_the_knife_edge():
    """VERDICT r5 item 1.  Policy: the device tries the unjittered matrix first and walks the reference's ladder only
    when a pivot of ITS factorisation is not positive, exactly like jit_cholesky around dpotrf.  Outside the knife-edge band the decision
    equals the reference's; inside it (the first exact pivot below tau = 8 max(n, 32) eps max K_ii lies within +-tau) either outcome is a
    correct execution of the reference's algorithm, the value of the nugget is zero or a ladder rung, and the decision is the same alone and
    in a batch."""
    X, t, thetas = adaptive_sweep_case()
    stats = adaptive_sweep_check(X, t, thetas, verbose=True)
    print(stats)
    # (no point of this sweep is "indefinite" in the strict sense -- a tiny positive pivot always comes before the first negative one; exactly
    # singular designs, where every implementation must jitter, are test_adaptive_jitter_ladder_on_duplicated_inputs / ..._mixed_batch_...)
    assert stats["definite"] >= 5 and stats["band"] >= 8 and stats["band_agree"] >= stats["band"] - 3


_SWEEP_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from test_gpu_parity import adaptive_sweep_case, adaptive_sweep_check
print("SWEEP-OK", adaptive_sweep_check(*adaptive_sweep_case()))
"""


@pytest.mark.parametrize("sched", ["mchol", "left", "la", "right"])
def test_adaptive_nugget_decision_sweep_under_every_schedule(sched):
    """The same sweep with the one-launch Cholesky forced and with each multi-launch schedule (the engine falls back to them after an
    abort and uses them for replica engines): the jitter decision follows the same policy under all of them, alone = in the batch."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _SWEEP_SCRIPT % {"root": root, "tests": os.path.join(root, "tests")}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MOGP_CHOL=sched), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SWEEP-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("tag", ["c1_n200_d4", "n500_d10"])
def test_default_priors_enter_posterior(tag):
    g = load_golden(tag + ".npz")
    gp = M.GaussianProcessGPU(g["X"], g["T"][1], nugget="fit")          # default priors computed on the host
    theta = g["defprior_theta"]
    assert_allclose(gp.logposterior(theta), g["defprior_logpost"], rtol=1e-8)
    assert_allclose(gp.logpost_deriv(theta), g["defprior_grad"], rtol=1e-7, atol=1e-7)
    pri = gp.priors
    assert np.isfinite(pri.get_logp(theta))
    assert len(pri.sample()) == gp.n_params


def test_variance_stability_regression():
    g = load_golden("var_stability.npz")
    gp = make_gp(g["x"], g["y"], nugget=1.e-8)
    gp.fit(g["theta"])
    mean, unc, _ = gp.predict(g["xt"])
    assert_allclose(unc, 0., atol=1e-3)            # tests/test_GaussianProcess.py:1144-1161
    assert np.all(unc >= 0.)
    assert_allclose(mean, g["mean"], rtol=1e-4, atol=1e-3)


def test_multioutput_vs_reference():
    g = load_golden("mogp4.npz")
    D = g["X"].shape[1]
    gp = M.MultiOutputGP_GPU(g["X"], g["T"], nugget=1e-6, priors=weak(D, 1e-6))
    assert gp.n_emulators == 4 and gp.get_indices_fit() == [] and gp.get_indices_not_fit() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        gp.predict(g["Xs"])
    gp.fit(g["thetas"])
    assert gp.get_indices_fit() == [0, 1, 2, 3]
    mean, unc, deriv = gp.predict(g["Xs"])
    assert mean.shape == (4, 40) and deriv.shape == (4, 40, 3)
    assert_allclose(mean, g["mean"], rtol=1e-7, atol=1e-9)
    assert_allclose(unc, g["var"], atol=1e-7)
    f, grad, ok = gp._mogp_gpu.eval(g["thetas"], grad=True)
    assert ok.all()
    assert_allclose(f, g["logpost"], rtol=1e-9)
    assert_allclose(grad, g["grad"], rtol=1e-7, atol=1e-8)
    # allow_not_fit: NaN rows (MultiOutputGP_GPU.py:292-296)
    gp.reset_fit_status()
    gp.fit_emulator(2, g["thetas"][2])
    mean, unc, deriv = gp.predict(g["Xs"], allow_not_fit=True)
    assert np.isnan(mean[0]).all() and np.isnan(unc[3]).all() and np.isnan(deriv[1]).all()
    assert_allclose(mean[2], g["mean"][2], rtol=1e-7, atol=1e-9)
    # the same emulator reached through emulator(i)
    em = gp.emulators[2]
    assert_allclose(em.predict(g["Xs"])[0], g["mean"][2], rtol=1e-7, atol=1e-9)


# ------------------------------------------------------------------------------------------------
# oracle on seeded inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kern", KERNELS)
def test_predict_deriv_vs_fd_and_oracle(kern):
    X, T, Xs = synth(11, 150, 3, 1, 20)
    theta = np.array([1.0, 0.5, 1.5, 0.3])
    gp = make_gp(X, T[0], kern, 1e-5)
    gp.fit(theta)
    mean, unc, deriv = gp.predict(Xs)
    ref = R.GPRef(X, T[0], kernel=kern, nugget=1e-5)
    ref.fit(theta)
    _, _, rd = ref.predict(Xs, deriv=True)
    assert_allclose(deriv, rd, rtol=1e-7, atol=1e-8)
    h = 1e-6                                         # reference style FD check, tests/test_GaussianProcess.py:1010-1015
    for d in range(3):
        e = np.zeros(3); e[d] = h
        fd = (gp.predict(Xs + e, unc=False, deriv=False)[0] - gp.predict(Xs - e, unc=False, deriv=False)[0]) / (2 * h)
        assert_allclose(deriv[:, d], fd, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kern", KERNELS)
def test_gradient_vs_finite_differences(kern):
    g = load_golden("grid11.npz")
    gp = make_gp(g["X"], g["t"], kern, "fit")
    th = np.array([-1., -1., -2., np.log(1e-6)])
    an = gp.logpost_deriv(th)
    h = 1e-6
    for p in range(4):
        e = np.zeros(4); e[p] = h
        fd = (gp.logposterior(th + e) - gp.logposterior(th - e)) / (2 * h)
        assert_allclose(an[p], fd, rtol=1e-4, atol=1e-4)      # the reference's bar, tests/test_GaussianProcess.py:626-661


def test_matern_nugget_fit_d20_vs_oracle():
    # C4-shaped (Matern-5/2, fitted nugget, d=20), at a size the oracle finishes in seconds
    X, T, Xs = synth(4, 700, 20, 1, 100)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(20))] * 20 + [0.2, np.log(1e-4)])
    gp = make_gp(X, T[0], "Matern52", "fit")
    ref = R.GPRef(X, T[0], kernel=R.MAT52, nugget="fit")
    assert_allclose(gp.logposterior(theta), ref.fit(theta), rtol=1e-10)
    assert_allclose(gp.logpost_deriv(theta), ref.logpost_deriv(theta), rtol=1e-7, atol=1e-8)
    mean, unc, _ = gp.predict(Xs, deriv=False)
    mu, var, _ = ref.predict(Xs)
    assert_allclose(mean, mu, rtol=1e-7, atol=1e-9)
    assert_allclose(unc, var, atol=1e-7 * np.exp(0.2))


def test_adaptive_jitter_ladder_on_duplicated_inputs():
    # exactly singular K (duplicated rows): both sides must walk the same ladder (linalg/cholesky.py:268-279)
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (40, 2)); X = np.vstack([X, X[:5]])
    t = np.sin(X.sum(axis=1))
    theta = np.array([0.5, 0.5, 1.0])
    gp = make_gp(X, t, nugget="adaptive")
    gp.fit(theta)
    ref = R.GPRef(X, t, nugget="adaptive")
    ref.fit(theta)
    assert gp.nugget > 0.
    assert_allclose(gp.nugget, ref.nugget, rtol=1e-13)
    assert_allclose(gp.current_logpost, ref.current_logpost, rtol=1e-6)
    # fixed zero nugget on the same matrix cannot be factorised -> RuntimeError (densegp_gpu.hpp:568-570)
    bad = make_gp(X, t, nugget=0.)
    with pytest.raises(RuntimeError, match="Unable to factorize"):
        bad.fit(theta)
    assert not bad.theta.data_has_been_set()


def test_adaptive_jitter_mixed_batch_two_stream_groups():
    # 24 emulators (two stream groups of 12) on duplicated inputs: exactly singular K, every emulator walks the ladder
    rng = np.random.default_rng(17)
    X = rng.uniform(0, 1, (150, 3)); X = np.vstack([X, X[:7]])
    B = 24
    T = np.stack([np.sin(X.sum(axis=1) + k) for k in range(B)])
    mo = M.MultiOutputGP_GPU(X, T, nugget="adaptive", priors=weak(3, "adaptive"))
    thetas = np.stack([np.r_[rng.uniform(-1., 1., 3), rng.uniform(-2., 2.)] for _ in range(B)])
    f, g, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    mo.fit(thetas)
    nug = mo._nuggets()
    assert np.all(nug > 0.)                     # exactly singular K: every emulator needs jitter
    for k in range(0, B, 5):
        ref = R.GPRef(X, T[k], nugget="adaptive")
        lp = ref.fit(thetas[k])
        assert_allclose(nug[k], ref.nugget, rtol=1e-12)
        assert_allclose(f[k], lp, rtol=1e-5)    # cond(K + jitter) ~ 1e6 / eps-level cancellations in the reference value
    # the same batch shape on a regular design with short length scales: zero jitter suffices for every emulator
    Xg = rng.uniform(0, 1, (157, 3))
    mg = M.MultiOutputGP_GPU(Xg, T, nugget="adaptive", priors=weak(3, "adaptive"))
    th = np.tile(np.r_[np.full(3, 6.), 0.], (B, 1))      # short length scales: well conditioned, zero jitter suffices
    fg, _, okg = mg._mogp_gpu.eval(th, grad=False)
    mg.fit(th)
    assert okg.all() and np.all(mg._nuggets() == 0.)


def test_error_behaviour_matches_reference():
    X, T, Xs = synth(5, 30, 2, 1, 4)
    gp = make_gp(X, T[0], nugget="fit")
    assert gp.n_params == 4 and gp.n == 30 and gp.D == 2 and gp.n_corr == 2 and gp.nugget_type == "fit"
    assert gp.Kinv_t is None and gp.current_logpost is None
    with pytest.raises(ValueError):
        gp.predict(Xs)                                   # GaussianProcessGPU.py:589-590
    with pytest.raises(RuntimeError):
        gp.fit(np.ones(3))                               # bad theta length, tests/test_GaussianProcess.py:346-347
    with pytest.raises(AssertionError):
        gp.logpost_deriv(np.ones(7))
    with pytest.raises(RuntimeError):
        gp.fit(np.array([800., 800., 800., 0.]))         # exp overflow -> factorisation fails
    gp.fit(np.zeros(4))
    with pytest.raises(AssertionError):
        gp.predict(np.zeros((3, 5)))
    small = make_gp(X, T[0], nugget=1e-6, max_batch_size=8)
    small.fit(np.zeros(3))
    out = np.zeros(20)
    with pytest.raises(RuntimeError, match="More test points"):      # densegp_gpu.hpp:312-315
        small._densegp_gpu.predict_batch(np.zeros((20, 2)), out)
    with pytest.raises(RuntimeError, match="too small"):             # densegp_gpu.hpp:307-310
        small._densegp_gpu.predict_batch(np.zeros((4, 2)), np.zeros(2))
    gp.theta = None
    assert not gp.theta.data_has_been_set()
    with pytest.raises(ValueError):
        M.GaussianProcessGPU(X, T[0], kernel="RationalQuadratic")
    with pytest.raises(ValueError):
        M.GaussianProcessGPU(X, T[0], nugget="nonsense")


def test_predict_chunking_ragged_and_single_point():
    X, T, Xs = synth(6, 120, 4, 1, 301)
    theta = np.array([0.5] * 4 + [0.1])
    gp = make_gp(X, T[0], nugget=1e-6, max_batch_size=64)     # 301 points -> 5 chunks, last ragged
    gp.fit(theta)
    ref = R.GPRef(X, T[0], nugget=1e-6); ref.fit(theta)
    mu, var, rd = ref.predict(Xs, deriv=True)
    mean, unc, deriv = gp.predict(Xs)
    assert_allclose(mean, mu, rtol=1e-8, atol=1e-10); assert_allclose(unc, var, atol=1e-8); assert_allclose(deriv, rd, rtol=1e-7, atol=1e-8)
    one = gp.predict(Xs[7])
    assert one.mean.shape == (1,) and one.deriv.shape == (1, 4)
    assert_allclose(one.mean, mu[7:8], rtol=1e-8)
    assert_allclose(gp(Xs[:3]), mu[:3], rtol=1e-8)
    assert gp.predict(Xs[:2], unc=False, deriv=False).unc is None
    # native single-point entry points (bindings.cu:71-95)
    v = np.zeros(1)
    assert_allclose(gp._densegp_gpu.predict(Xs[3]), mu[3], rtol=1e-8)
    assert_allclose(gp._densegp_gpu.predict_variance(Xs[3], v), mu[3], rtol=1e-8)
    assert_allclose(v[0] + 1e-6, var[3], atol=1e-8)
    # 1-D inputs
    g1 = make_gp(X[:, 0], T[0], nugget=1e-4); g1.fit(np.array([1., 0.]))
    r1 = R.GPRef(X[:, 0], T[0], nugget=1e-4); r1.fit(np.array([1., 0.]))
    assert_allclose(g1.predict(np.linspace(0, 1, 7))[0], r1.predict(np.linspace(0, 1, 7))[0], rtol=1e-8, atol=1e-10)


def test_getters_invq_cholesky_layout():
    X, T, _ = synth(7, 90, 3, 1, 1)
    theta = np.array([0.2, 0.4, 0.6, 0.5])
    gp = make_gp(X, T[0], nugget=1e-3); gp.fit(theta)
    K = gp.get_K_matrix() + 1e-3 * np.eye(90)
    L = gp.L
    assert_allclose(L @ L.T, K, rtol=1e-12, atol=1e-13)
    assert np.all(np.triu(L, 1) == 0.)
    raw = np.zeros((90, 90)); gp._densegp_gpu.get_cholesky_lower(raw)
    assert_allclose(np.tril(raw.T), L)                          # GaussianProcessGPU.py:476-478 convention
    Q = np.zeros((90, 90)); gp._densegp_gpu.get_invQ(Q)
    assert_allclose(Q @ K, np.eye(90), atol=1e-8)
    assert_allclose(Q, Q.T, atol=0)
    assert_allclose(gp.Kinv_t, np.linalg.solve(K, T[0]), rtol=1e-8)
    th = gp.theta
    assert_allclose(th.get_data(), theta); assert_allclose(th.get_cov(), np.exp(0.5)); assert th.get_nugget_size() == 1e-3


def test_mean_functions_follow_gpu_reference_semantics():
    # mean parameters are part of theta (densegp_gpu.hpp:497-508); oracle = zero-mean GP on t - m(X)
    X, T, Xs = synth(8, 80, 2, 1, 9)
    theta_k = np.array([0.3, 0.7, 0.2])
    gp = M.GaussianProcessGPU(X, T[0], mean="1.5", nugget=1e-5, priors=weak(2, 1e-5))
    gp.fit(theta_k)
    ref = R.GPRef(X, T[0] - 1.5, nugget=1e-5); ref.fit(theta_k)
    assert_allclose(gp.current_logpost, ref.current_logpost, rtol=1e-10)
    assert_allclose(gp.predict(Xs)[0], ref.predict(Xs)[0] + 1.5, rtol=1e-8)
    gp = M.GaussianProcessGPU(X, T[0], mean="c+c*x[0]+c*x[1]^2", nugget=1e-5, priors=weak(2, 1e-5))
    beta = np.array([0.4, -0.3, 0.8])
    assert gp.n_params == 6
    full = np.concatenate([beta, theta_k])
    mX = beta[0] + beta[1] * X[:, 0] + beta[2] * X[:, 1] ** 2
    ref = R.GPRef(X, T[0] - mX, nugget=1e-5)
    assert_allclose(gp.logposterior(full), ref.fit(theta_k), rtol=1e-10)
    grad = gp.logpost_deriv(full)
    assert_allclose(grad[3:], ref.logpost_deriv(theta_k), rtol=1e-7, atol=1e-8)
    h = 1e-6
    for p in range(3):
        e = np.zeros(6); e[p] = h
        fd = (gp.logposterior(full + e) - gp.logposterior(full - e)) / (2 * h)
        assert_allclose(grad[p], fd, rtol=1e-5, atol=1e-5)
    gp.fit(full)
    mXs = beta[0] + beta[1] * Xs[:, 0] + beta[2] * Xs[:, 1] ** 2
    mean, _, deriv = gp.predict(Xs)
    assert_allclose(mean, ref.predict(Xs)[0] + mXs, rtol=1e-8)
    _, _, rd = ref.predict(Xs, deriv=True)
    rd = rd + np.stack([np.full(9, beta[1]), 2 * beta[2] * Xs[:, 1]], axis=1)
    assert_allclose(deriv, rd, rtol=1e-7, atol=1e-8)


def test_pickle_roundtrip_refits():
    X, T, Xs = synth(9, 60, 2, 1, 5)
    gp = make_gp(X, T[0], "Matern52", 1e-5); gp.fit(np.array([0.1, 0.2, 0.3]))
    clone = pickle.loads(pickle.dumps(gp))
    assert_allclose(clone.predict(Xs)[0], gp.predict(Xs)[0], rtol=0, atol=0)
    assert clone.kernel == gp.kernel and clone.nugget == gp.nugget


@pytest.mark.parametrize("mean, analytic", [("c", False), ("c+c*x[0]+c*x[1]^2", False), ("c+c*x[0]", True), (0.75, False)])
def test_pickle_keeps_mean_function_analytic_flag_and_current_nugget(mean, analytic):
    """The state is inputs, targets, kernel, priors, theta AND the mean function, analytic_mean and the nugget as it is
    now (the reference pickles its whole __dict__): a clone predicts exactly what the original does."""
    X, T, Xs = synth(11, 70, 2, 1, 9)
    t = T[0] + 3.0 + 2.0 * X[:, 0]
    native = LibGPGPU.FixedMeanFunc(mean) if isinstance(mean, float) else mean
    gp = M.GaussianProcessGPU(X, t, mean=native, kernel="Matern52", nugget=1e-5, analytic_mean=analytic,
                              priors=GPPriors(n_corr=2, nugget_type="fixed"))
    gp.nugget = 3e-4                     # changed after construction: the clone must carry 3e-4, not 1e-5
    rng = np.random.default_rng(0)
    gp.fit(rng.normal(size=gp.n_params) * 0.3)
    clone = pickle.loads(pickle.dumps(gp))
    assert clone.n_params == gp.n_params and clone.nugget == 3e-4 and clone.nugget_type == "fixed"
    assert clone._analytic_mean == analytic
    a, b = gp.predict(Xs), clone.predict(Xs)
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.unc, b.unc)
    assert clone.current_logpost == gp.current_logpost
    # an adaptive nugget pickles as "adaptive", not as the jitter it found
    gq = M.GaussianProcessGPU(X, t, mean=native, analytic_mean=analytic)
    gq.fit(np.zeros(gq.n_params))
    cq = pickle.loads(pickle.dumps(gq))
    assert cq.nugget_type == "adaptive" and np.array_equal(cq.predict(Xs).mean, gq.predict(Xs).mean)


def test_native_prior_objects_are_not_silently_weakened():
    """LibGPGPU re-exports the native prior classes; handing one of them to GPPriors keeps its type and parameters
    (they used to fall through to the weak prior), and an unknown prior class is a TypeError."""
    from mogp_emulator_amd.GaussianProcessGPU import _native_prior
    from mogp_emulator_amd import libgpgpu
    assert _native_prior(libgpgpu.InvGammaPrior(2., 3.)) == (LibGPGPU.prior_type.InvGamma, [2., 3.])
    assert _native_prior(libgpgpu.GammaPrior(2., 3.)) == (LibGPGPU.prior_type.Gamma, [2., 3.])
    assert _native_prior(libgpgpu.LogNormalPrior(2., 3.)) == (LibGPGPU.prior_type.LogNormal, [2., 3.])
    assert _native_prior(InvGammaPrior(2., 3.)) == (LibGPGPU.prior_type.InvGamma, [2., 3.])
    assert _native_prior(None)[0] == LibGPGPU.prior_type.Weak and _native_prior(libgpgpu.WeakPrior())[0] == LibGPGPU.prior_type.Weak

    class Strange(libgpgpu.WeakPrior):
        pass
    with pytest.raises(TypeError):
        _native_prior(Strange())


def test_set_gppriors_with_a_constructed_container():
    """DenseGP_GPU.set_gppriors(GPPriors(n_corr, nugget_type)) (bindings.cu:62-65, 528-556): the distributions of the host
    container end up inside the native emulator -- its prior view returns the container's numbers, the log-posterior
    moves by exactly the log-prior, and the cached posterior is not served stale."""
    from mogp_emulator_amd import libgpgpu as L
    rng = np.random.default_rng(8)
    X = rng.uniform(0, 1, (60, 2)); t = np.sin(X.sum(axis=1))
    gp = make_gp(X, t, nugget="fit")
    theta = np.array([0.5, 1.0, 0.3, np.log(1e-3)])
    lp_weak = gp.logposterior(theta)
    pri = L.GPPriors(2, L.nugget_type.fit)
    pri.create_corr_priors([(L.prior_type.InvGamma, [2., 1.]), (L.prior_type.Gamma, [3., .5])])
    pri.create_cov_prior((L.prior_type.LogNormal, [.7, 1.3]))
    pri.set_nugget((L.prior_type.InvGamma, [3.3, 4.3e-4]))
    gp._densegp_gpu.set_gppriors(pri)
    th = L.GPParameters(0, 2, L.nugget_type.fit); th.set_data(theta)
    view = gp._densegp_gpu.get_gppriors()
    assert_allclose(view.get_logp(th), pri.get_logp(th), rtol=1e-13)
    assert_allclose(view.get_dlogpdtheta(th), pri.get_dlogpdtheta(th), rtol=1e-13)
    assert_allclose(gp.logposterior(theta), lp_weak - pri.get_logp(th), rtol=1e-12)
    with pytest.raises(RuntimeError):
        gp._densegp_gpu.set_gppriors(view)                 # a view is not a container
    with pytest.raises(RuntimeError):
        view.set_cov()


# ------------------------------------------------------------------------------------------------
# fit_GP_MAP
# ------------------------------------------------------------------------------------------------
def test_fit_GP_MAP_single_reaches_reference_optimum():
    g = load_golden("fitmap_c1.npz")
    LibGPGPU.set_fit_options(max_iter=500, ftol=1e-12, gtol=1e-8, seed=7)
    gp = M.GaussianProcessGPU(g["X"], g["t"], nugget=1e-6)         # default priors, as in the golden run
    gp = M.fit_GP_MAP(gp, n_tries=1, theta0=g["theta0"])
    assert gp.theta.data_has_been_set()
    # trajectory parity is unpinned; the MAP objective must be at least as good as scipy's end point
    assert gp.current_logpost <= g["logpost_hat"] + 1e-5 * abs(g["logpost_hat"])
    assert_allclose(gp.logposterior(g["theta_hat"]), g["logpost_hat"], rtol=1e-8)
    gp.fit(g["theta_hat"])
    assert_allclose(gp.predict(g["Xs"])[0], g["mean"], rtol=1e-6, atol=1e-7)
    LibGPGPU.set_fit_options(max_iter=200, ftol=1e-9, gtol=1e-6, seed=0)


def test_fit_GP_MAP_multioutput_and_failures():
    X, T, Xs = synth(10, 100, 3, 6, 12)
    LibGPGPU.set_fit_options(seed=11)
    gp = M.fit_GP_MAP(X, T, nugget=1e-6, n_tries=2)
    assert isinstance(gp, M.MultiOutputGP_GPU) and gp.get_indices_not_fit() == []      # tests/test_fitting.py:45-65
    mean, unc, _ = gp.predict(Xs)
    assert mean.shape == (6, 12) and np.all(np.isfinite(mean)) and np.all(unc >= 0.)
    # each emulator's optimum must beat its own starting objective
    th0 = np.zeros(4)
    gp2 = M.MultiOutputGP_GPU(X, T, nugget=1e-6)
    f0, _, _ = gp2._mogp_gpu.eval(np.tile(th0, (6, 1)), grad=False)
    gp2 = M.fit_GP_MAP(gp2, n_tries=1, theta0=th0)
    f1 = np.array([em.current_logpost for em in gp2.emulators])
    assert np.all(f1 < f0)
    with pytest.raises(NotImplementedError):
        M.fit_GP_MAP(gp2, method="CG", refit=True)
    # a hopeless start (theta0 = 800: overflow) with a single try leaves every emulator unfit
    gp3 = M.MultiOutputGP_GPU(X, T[:2], nugget=1e-6)
    gp3 = M.fit_GP_MAP(gp3, n_tries=1, theta0=np.full(4, 800.))
    assert gp3.get_indices_not_fit() == [0, 1]
    with pytest.raises(RuntimeError):
        M.fit_GP_MAP(gp3, n_tries=1, theta0=np.full(4, 800.), skip_failures=False)
    single = M.GaussianProcessGPU(X, T[0], nugget=1e-6)
    with pytest.raises(RuntimeError):
        M.fit_GP_MAP(single, n_tries=1, theta0=np.full(4, 800.))
    with pytest.raises(RuntimeError):
        M.fit_GP_MAP(single, n_tries=1, theta0=np.zeros(9))      # wrong theta0 length, tests/test_fitting.py:135-136


# ------------------------------------------------------------------------------------------------
# BASELINE sizes: oracle where it finishes in seconds + size-independent identities
# ------------------------------------------------------------------------------------------------
def test_c2_full_size_vs_oracle_and_identities():
    n, d = 2000, 10
    X, T, Xs = synth(20240607 + 2, n, d, 8, 700)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
    eta = 1e-6
    mo = M.MultiOutputGP_GPU(X, T, nugget=eta, priors=weak(d, eta))
    f, g, ok = mo._mogp_gpu.eval(np.tile(theta, (8, 1)), grad=True)
    assert ok.all()
    ref = R.GPRef(X, T[0], nugget=eta)
    assert_allclose(f[0], ref.fit(theta), rtol=1e-10)
    assert_allclose(g[0], ref.logpost_deriv(theta), rtol=1e-7, atol=1e-7)
    mean, unc, _ = mo.predict(Xs, deriv=False)
    mu, var, _ = ref.predict(Xs)
    assert_allclose(mean[0], mu, rtol=1e-7, atol=1e-8)
    assert_allclose(unc[0], var, atol=1e-7)
    # identities, all 8 emulators: at a training point x_i the predictive mean is t_i - eta*alpha_i and the
    # (nugget-free) variance is eta - eta^2 [ (K+eta I)^-1 ]_ii
    tm, tv, _ = mo.predict(X[:256], deriv=False, include_nugget=False)
    for k in range(8):
        em = mo.emulators[k]
        a = em.Kinv_t
        assert_allclose(tm[k], T[k, :256] - eta * a[:256], rtol=1e-7, atol=1e-8)
    Q = np.zeros((n, n)); mo._mogp_gpu.emulator(3).get_invQ(Q)
    assert_allclose(tv[3], np.maximum(eta - eta ** 2 * np.diag(Q)[:256], 0.), atol=1e-9)
    L = mo.emulators[5].L
    K = mo.emulators[5].get_K_matrix()
    resid = np.abs(L @ L.T - K - eta * np.eye(n)).max()
    assert resid < 1e-12
    assert np.abs(K @ mo.emulators[5].Kinv_t + eta * mo.emulators[5].Kinv_t - T[5]).max() < 1e-8
    # batching is invisible up to rounding: an emulator inside the batch equals the same emulator alone.  (The Cholesky
    # schedule is chosen by batch x size and the schedules group the panel updates differently; with one schedule forced
    # the two are bit-identical, see test_cholesky_schedules_and_switches.)
    mo.fit(np.tile(theta, (8, 1)))               # same code path (fit: alpha by back substitution) on both sides
    solo = make_gp(X, T[2], nugget=eta); solo.fit(theta)
    assert_allclose(solo.current_logpost, mo.emulators[2].current_logpost, rtol=1e-10)
    assert_allclose(solo.Kinv_t, mo.emulators[2].Kinv_t, rtol=1e-6, atol=1e-6 * np.abs(solo.Kinv_t).max())


_SWITCH_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd.Priors import GPPriors
from oracle import cpu_ref as R
from test_gpu_parity import synth, weak, make_gp
n, d = 2000, 10
X, T, Xs = synth(20240607 + 2, n, d, 8, 300)
theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
eta = 1e-6
mo = M.MultiOutputGP_GPU(X, T, nugget=eta, priors=weak(d, eta))
f, g, ok = mo._mogp_gpu.eval(np.tile(theta, (8, 1)), grad=True)
assert ok.all()
ref = R.GPRef(X, T[0], nugget=eta)
np.testing.assert_allclose(f[0], ref.fit(theta), rtol=1e-10)
np.testing.assert_allclose(g[0], ref.logpost_deriv(theta), rtol=1e-7, atol=1e-7)
mean, unc, _ = mo.predict(Xs, deriv=False)
mu, var, _ = ref.predict(Xs)
np.testing.assert_allclose(mean[0], mu, rtol=1e-7, atol=1e-8)
np.testing.assert_allclose(unc[0], var, atol=1e-7)
mo.fit(np.tile(theta, (8, 1)))
solo = make_gp(X, T[2], nugget=eta); solo.fit(theta)
if %(bitwise)r:      # one schedule for every batch size: an emulator inside a batch equals the same emulator alone, bit for bit
    assert solo.current_logpost == mo.emulators[2].current_logpost
    assert np.array_equal(solo.Kinv_t, mo.emulators[2].Kinv_t)
import hashlib
digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in (f, g, mean, unc, solo.Kinv_t, mo.emulators[2].Kinv_t))).hexdigest()
print("SWITCH-OK", repr(float(f[0])), "DIGEST", digest)
"""

# Switches the library no longer reads (retired in round 7 with the kernel paths only they reached, HISTORY.md).  A process that still sets one
# computes what the default computes, bit for bit; the branches they used to force, where they still exist, are reached by the default-path
# tests (test_c3_full_batch_64_default_schedule_vs_oracle, test_c2_single_output_fit_and_predict_at_all_10k_points_vs_oracle, the C2 script here).
_RETIRED_SWITCHES = [{"MOGP_CHOL": "mchol", "MOGP_MC_WGS": "2"}, {"MOGP_MCHOL": "0"}, {"MOGP_CHOL": "mchol", "MOGP_MC_SOLO": "0"},
                     {"MOGP_TRTRI_WT4_FROM": "128"}, {"MOGP_TRTRI_WT4_FROM": "100000"}, {"MOGP_KINV_WT": "2"}, {"MOGP_KINV_WT": "4"},
                     {"MOGP_CHOL": "mchol", "MOGP_MC_AHEAD": "0"}, {"MOGP_CHOL": "mchol", "MOGP_MC_EGRP": "0"},
                     {"MOGP_CHOL": "mchol", "MOGP_MC_EGRP": "1", "MOGP_MC_WGS": "2"}, {"MOGP_BS_HOIST": "0"}, {"MOGP_BS_LOGDET": "0"},
                     {"MOGP_CHOL": "mchol", "MOGP_MC_URG": "0"}, {"MOGP_CHOL": "mchol", "MOGP_MC_URG": "1", "MOGP_MC_WGS": "2"},
                     {"MOGP_PV_SINGLE": "1"}, {"MOGP_PV_SINGLE": "0"}, {"MOGP_PV_Q": "0"}, {"MOGP_PV_Q": "1", "MOGP_PV_SINGLE": "0"},
                     {"MOGP_BACKSOLVE": "1"}, {"MOGP_BS_SENTINEL": "0"}]
_SWITCH_DEFAULT = {}


def _run_switch_script(env):
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bitwise = env.get("MOGP_CHOL") in ("mchol", "la", "left", "right")
    script = _SWITCH_SCRIPT % {"root": root, "tests": os.path.join(root, "tests"), "bitwise": bitwise}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SWITCH-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.split("DIGEST")[-1].split()[0]


@pytest.mark.parametrize("env", [{"MOGP_CHOL": "mchol"}, {"MOGP_CHOL": "la"}, {"MOGP_CHOL": "left"}, {"MOGP_CHOL": "right"}, {"MOGP_CHOL": "multi"},
                                 {"MOGP_KS_BUDGET_GB": "0.05"}] + _RETIRED_SWITCHES,
                         ids=lambda e: ",".join(k + "=" + v for k, v in e.items()))
def test_cholesky_schedules_and_switches(env):
    """Every forced Cholesky schedule and the cross-covariance chunking switch libmogp_hip.so reads go through the C2
    full-size parity check in its own process (the library reads its environment once); with ONE schedule forced, batching is bit-invisible
    (multi: the multi-launch schedule of each regime -- the batch and the solo fit take different ones).  A retired switch passes the same
    check and changes no bit of the default's results."""
    digest = _run_switch_script(env)
    if env in _RETIRED_SWITCHES:
        if "default" not in _SWITCH_DEFAULT:
            _SWITCH_DEFAULT["default"] = _run_switch_script({})
        assert digest == _SWITCH_DEFAULT["default"], "a retired switch changed the results: %r" % env


def test_diagonal_block_grouped_columns_vs_column_at_a_time(tmp_path):
    """the 128 x 128 diagonal block factors four columns per MFMA through an explicit 4 x 4 inverse (chol128_dev.h
    c128_column_groups, round 4); the column-at-a-time form it replaced is still in the header behind -DC128_RANK1.  Both are built into
    the stand-alone probe (tools/chol128_probe.hip) and factor the same blocks: backward error max|L L^T - A| / max|A| of each against a
    host Cholesky on well-conditioned blocks (tight bar) and on nearly singular ones (shift 1e-10 on a rank-64 Gram matrix), where the
    grouped form may cost a small factor but not an order of magnitude."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, flags in (("grouped", []), ("rank1", ["-DC128_RANK1"])):
        exe = str(tmp_path / ("probe_" + tag))
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1"] + flags +
                              ["-I", os.path.join(root, "mogp_emulator_amd", "csrc"), os.path.join(root, "tools", "chol128_probe.hip"), "-o", exe],
                              stderr=subprocess.DEVNULL)
        for case, args in (("well", ["16", "8.0", "128"]), ("ill", ["16", "1e-10", "64"])):
            out = subprocess.check_output([exe] + args, timeout=120).decode()
            m = re.search(r"backward error.*device ([0-9.e+-]+), host Cholesky ([0-9.e+-]+)", out)
            assert m, out[-500:]
            res[(tag, case)] = (float(m.group(1)), float(m.group(2)))
    for tag in ("grouped", "rank1"):
        dev, host = res[(tag, "well")]
        assert dev <= 1e-14 and dev <= 4 * host, (tag, res)
    g, r1 = res[("grouped", "ill")][0], res[("rank1", "ill")][0]
    assert g <= 1e-13 and g <= 16 * max(r1, res[("grouped", "ill")][1]), res


def test_predictive_variance_on_ragged_shapes():
    """Odd numbers of row tiles (a pair with one tile), partial super-tiles, batches that are not a multiple of 8: the variances of
    the first and the last emulator against the oracle."""
    for n, d, B, m in ((600, 3, 3, 700), (129, 2, 1, 130), (900, 5, 16, 1100), (1300, 4, 5, 260)):
        X, T, Xs = synth(900 + n, n, d, B, m)
        theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
        mo = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=weak(d, 1e-6))
        mo.fit(np.tile(theta, (B, 1)))
        mean, unc, _ = mo.predict(Xs, deriv=False)
        for k in (0, B - 1):
            ref = R.GPRef(X, T[k], nugget=1e-6); ref.fit(theta)
            mu, var, _ = ref.predict(Xs)
            assert_allclose(mean[k], mu, rtol=1e-7, atol=1e-8)
            assert_allclose(unc[k], var, atol=1e-7)


_BS_TIMEOUT_SCRIPT = r"""
import sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd import _capi
from oracle import cpu_ref as R
from test_gpu_parity import synth, weak
n, d, B = 1500, 6, 5
X, T, Xs = synth(77, n, d, B, 50)
theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
for kern, nugget in (("SquaredExponential", 1e-6), ("Matern52", "adaptive")):    # (Matern: factorises without jitter on both sides)
    mo = M.MultiOutputGP_GPU(X, T, kernel=kern, nugget=nugget, priors=weak(d, nugget))
    f, _, ok = mo._mogp_gpu.eval(np.tile(theta, (B, 1)), grad=False)
    assert ok.all()
    mo.fit(np.tile(theta, (B, 1)))
    for k in (0, B - 1):
        ref = R.GPRef(X, T[k], kernel=kern, nugget=nugget)
        np.testing.assert_allclose(f[k], ref.fit(theta), rtol=1e-9)
        np.testing.assert_allclose(mo.emulators[k].Kinv_t, ref.Kinv_t, rtol=1e-5, atol=1e-6 * np.abs(ref.Kinv_t).max())
        # a timeout must NOT start the jitter ladder: the adaptive nugget stays what the oracle finds (0 here)
        np.testing.assert_allclose(mo.emulators[k].nugget, ref.nugget, rtol=1e-12, atol=0)
c = ctypes.c_longlong()
assert _capi.load().mogp_profile_counter(b"backsolve_timeouts", ctypes.byref(c)) == 0
print("BS-TIMEOUTS", c.value)
"""


_MC_ABORT_SCRIPT = r"""
import sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd import _capi
from oracle import cpu_ref as R
from test_gpu_parity import synth, weak, make_gp
n, d, B = 1500, 6, 5
X, T, Xs = synth(78, n, d, B, 50)
theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
mo = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=weak(d, 1e-6))
f, g, ok = mo._mogp_gpu.eval(np.tile(theta, (B, 1)), grad=True)      # deferred status: the abort word comes back with the log-determinants
assert ok.all()
mo.fit(np.tile(theta, (B, 1)))
solo = make_gp(X, T[1], nugget=1e-6); solo.fit(theta)                # fit(): status read right after the factorisation
# cond(K) = 6e8 here: LAPACK's own log-posterior is 1e-11 ... 5e-10 (relative) from the exact value of this fp64 matrix, and two
# backward-stable factorisations differ by as much.  So the bar is the EXACT value (80-bit long double, oracle/exact.py), for the
# device and for the oracle alike, at 0.02 cond(K) eps = 2.8e-9.
from oracle.exact import loglike_longdouble, cond_eps
ref = R.GPRef(X, T[0], nugget=1e-6); ref.fit(theta)
Kn = ref.get_K_matrix() + 1e-6 * np.eye(n)
tol = 0.02 * cond_eps(Kn)
assert 1e-9 < tol < 1e-8, tol
like = loglike_longdouble(Kn, T)
for k in range(B):
    ref = R.GPRef(X, T[k], nugget=1e-6)
    fo = ref.fit(theta)
    prior = fo - 0.5 * (np.dot(ref.t, ref.Kinv_t) + R.logdet_L(ref.L) + n * np.log(2. * np.pi))
    exact = float(like[k] + np.longdouble(prior))
    np.testing.assert_allclose(fo, exact, rtol=tol)
    np.testing.assert_allclose(f[k], exact, rtol=tol)
    if k in (0, B - 1):
        np.testing.assert_allclose(g[k], ref.logpost_deriv(theta), rtol=1e-7, atol=1e-7)
        np.testing.assert_allclose(mo.emulators[k].Kinv_t, ref.Kinv_t, rtol=1e-6, atol=1e-7 * np.abs(ref.Kinv_t).max())
np.testing.assert_allclose(solo.current_logpost, mo.emulators[1].current_logpost, rtol=tol)
c = ctypes.c_longlong()
assert _capi.load().mogp_profile_counter(b"mchol_aborts", ctypes.byref(c)) == 0
print("MC-ABORTS", c.value)
"""


def test_one_launch_cholesky_abort_falls_back_to_the_multi_launch_schedule():
    """Every wait inside the one-launch Cholesky (kernels_mchol.hip) is bounded; when one gives up the kernel sets its abort
    word, every workgroup leaves, and the engine must factorise again with a multi-launch schedule.  MOGP_MC_SPIN=0 makes
    the first unsatisfied wait a timeout, so the fallback runs in every evaluation: results must still be the oracle's."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _MC_ABORT_SCRIPT % {"root": root, "tests": os.path.join(root, "tests")}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MOGP_CHOL="mchol", MOGP_MC_SPIN="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MC-ABORTS" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("MC-ABORTS")[1].split()[0]) > 0, "the forced timeouts never happened: the fallback was not exercised"


def test_c5_like_conditioning_against_the_exact_value():
    """at n = 16000 nothing independent of LAPACK can be computed in full, so the same family one size down, where it
    can: n = 4000, d = 8, C5's theta and nugget.  The device AND the oracle against the likelihood of the same fp64 matrix evaluated
    in 80-bit long double (oracle/exact.py), at 0.02 cond(K) eps -- the bar of the n = 1500 test -- and each factor's own long-double
    value (loglike_from_factor_longdouble) against its fp64 result at 1e-11."""
    from oracle.exact import loglike_longdouble, loglike_from_factor_longdouble, cond_eps
    n, d = 4000, 8
    X, T, Xs = synth(20240607 + 5, n, d, 2, 16)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
    eta = 1e-6
    ref = R.GPRef(X, T[0], nugget=eta); ref.fit(theta)
    Kn = ref.get_K_matrix() + eta * np.eye(n)
    ce = cond_eps(Kn)
    tol = 0.02 * ce
    like = loglike_longdouble(Kn, T, nb=128)
    for k in range(2):
        gp = make_gp(X, T[k], nugget=eta)
        f_dev = gp.logposterior(theta)
        gp.fit(theta)
        rk = R.GPRef(X, T[k], nugget=eta)
        f_ref = rk.fit(theta)
        prior = f_ref - 0.5 * (np.dot(rk.t, rk.Kinv_t) + R.logdet_L(rk.L) + n * np.log(2. * np.pi))
        exact = float(like[k] + np.longdouble(prior))
        assert_allclose(f_ref, exact, rtol=tol)
        assert_allclose(f_dev, exact, rtol=tol)
        own = float(loglike_from_factor_longdouble(gp.L, T[k]) + np.longdouble(prior))
        assert abs(f_dev - own) <= 1e-11 * abs(own), (f_dev, own)
        print("n=4000 k=%d: cond eps %.2e; (oracle - exact)/exact %.2e, (device - exact)/exact %.2e, device vs its own factor %.2e" % (
            k, ce, (f_ref - exact) / exact, (f_dev - exact) / exact, (f_dev - own) / own))


def test_in_kernel_hand_offs_are_bit_stable_under_uneven_load():
    """The hand-offs inside the one-launch Cholesky and the chained back substitution (write-through stores, drained, then a relaxed
    agent-scope flag; consumers never touch an address before its final value is published) rest on an argument, not on acquire /
    release fences.  This is the mechanical check MI355X_MICROARCH.md prescribes: every hand-off under UNEVEN load, every
    word compared.  Both kernels are bit-reproducible by construction (fixed k order per tile), so ONE stale word anywhere shows up as a bit
    difference: 150 evaluations of 24 x n=1000 (three per XCD queue, two workgroups per CU) and 150 of 3 x n=1300 (single queue, one workgroup
    per CU) while a second engine on another stream keeps part of the chip busy with predictions of varying size; the log-posteriors,
    alpha and the whole factor of two emulators must equal the undisturbed first evaluation bit for bit, and no launch may have aborted."""
    import ctypes
    import threading
    lib = _capi.load()

    def aborts():
        c = ctypes.c_longlong()
        lib.mogp_profile_counter(b"mchol_aborts", ctypes.byref(c))
        t = ctypes.c_longlong()
        lib.mogp_profile_counter(b"backsolve_timeouts", ctypes.byref(t))
        return c.value + t.value
    Xn, Tn, Xsn = synth(77, 1500, 6, 6, 3000)
    noise = M.MultiOutputGP_GPU(Xn, Tn, nugget=1e-6, priors=weak(6, 1e-6))
    noise.fit(np.tile(np.array([1.0] * 6 + [0.]), (6, 1)))
    stop = threading.Event()

    def make_noise():
        k = 0
        while not stop.is_set():
            m = (300, 3000, 900, 1700)[k % 4]                       # bursts of different length: the load on the CUs keeps changing
            noise.predict(Xsn[:m], deriv=False)
            k += 1
    a0 = aborts()
    for n, d, B in ((1000, 5, 24), (1300, 4, 3)):
        X, T, _ = synth(500 + n, n, d, B, 4)
        theta = np.tile(np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.]), (B, 1)) + 0.02 * np.arange(B)[:, None]
        mo = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=weak(d, 1e-6))

        def snapshot():
            f, _, ok = mo._mogp_gpu.eval(theta, grad=False)
            assert ok.all()
            mo.fit(theta)
            return f.copy(), [mo.emulators[k].L.copy() for k in (0, B - 1)], [mo.emulators[k].Kinv_t.copy() for k in (0, B - 1)]
        f0, L0, a0_ = snapshot()
        th = threading.Thread(target=make_noise)
        th.start()
        try:
            for it in range(150):
                f, L, a = snapshot()
                assert np.array_equal(f, f0), "log-posterior differs in evaluation %d (n=%d)" % (it, n)
                for k in range(2):
                    assert np.array_equal(L[k], L0[k]), "factor differs in evaluation %d (n=%d)" % (it, n)
                    assert np.array_equal(a[k], a0_[k]), "alpha differs in evaluation %d (n=%d)" % (it, n)
        finally:
            stop.set()
            th.join()
            stop.clear()
    assert aborts() == a0, "a bounded wait gave up under load"


def test_backsolve_chain_timeout_is_retried_not_reported_as_failure():
    """a wait of the one-launch back substitution that gives up must not look like a failed
    factorisation.  MOGP_BS_SPIN=0 turns every wait that is not satisfied at the first poll into a timeout; the engine has
    to notice (status word of its own), repeat those solves with the multi-launch path and return the oracle's numbers --
    fixed and adaptive nugget (no jitter may be added)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _BS_TIMEOUT_SCRIPT % {"root": root, "tests": os.path.join(root, "tests")}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MOGP_BS_SPIN="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "BS-TIMEOUTS" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert int(out.stdout.split("BS-TIMEOUTS")[1].split()[0]) > 0, "the forced timeouts never happened: the test did not exercise the fallback"


def test_objective_with_and_without_gradient_is_the_same_number():
    """Round 6: eval(grad=True) takes alpha from the same one-launch back substitution as eval(grad=False) (it runs under the triangular
    inversion on a second stream) instead of from a product with L^-1: log-posterior and K^-1 t agree BIT FOR BIT between the two calls --
    what the line search of fit_GP_MAP compares (objective of a trial point first, its gradient later) is one number.  1, 9 and 64 emulators."""
    for B, n in ((1, 900), (9, 700), (64, 300)):
        X, T, _ = synth(31 + B, n, 4, B, 4)
        mo = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=weak(4, 1e-6))
        theta = np.tile(np.array([1.5, 2., 1., 2.5, 0.3]), (B, 1)) + 0.01 * np.arange(B)[:, None]
        f0, _, ok0 = mo._mogp_gpu.eval(theta, grad=False)
        mo.fit(theta)
        a0 = [mo.emulators[k].Kinv_t.copy() for k in (0, B - 1)]
        f1, g1, ok1 = mo._mogp_gpu.eval(theta, grad=True)
        assert ok0.all() and ok1.all() and np.all(np.isfinite(g1))
        assert np.array_equal(f0, f1), np.abs(f0 - f1).max()
        mo2 = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=weak(4, 1e-6))
        mo2._mogp_gpu.eval(theta, grad=True)
        for k, a in zip((0, B - 1), a0):
            b = np.zeros(n); mo2._mogp_gpu.emulator(k).get_invQt(b)
            assert np.array_equal(a, b)
        ref = R.GPRef(X, T[0], nugget=1e-6)
        assert_allclose(f1[0], ref.fit(theta[0]), rtol=1e-9)
        assert_allclose(g1[0], ref.logpost_deriv(theta[0]), rtol=1e-6, atol=1e-7)


def test_non_finite_targets_are_not_reported_as_a_chain_timeout():
    """a legitimately non-finite alpha (NaN / inf targets) used to look like a timed-out wait of the one-launch back
    substitution (any NaN in the leftmost chunk's result set the time-out status): counted in `backsolve_timeouts`, re-solved by the
    multi-launch path on every evaluation.  The time-out now has a channel of its own: such targets give a non-finite log-posterior, as
    on the CPU (GaussianProcess.py:657-685 propagates them), and the counter stays where it was -- for 1, 9 and 70 emulators (one / two
    workgroups per CU), the bad value in the first, a middle and the last chunk of the chain."""
    import ctypes
    lib = _capi.load()

    def timeouts():
        c = ctypes.c_longlong()
        lib.mogp_profile_counter(b"backsolve_timeouts", ctypes.byref(c))
        return c.value
    for B, n in ((1, 700), (9, 700), (70, 400)):
        X, T, _ = synth(5 + B, n, 3, B, 4)
        bad = {0: (5, np.nan), B // 2: (n // 2, np.inf), B - 1: (n - 1, np.nan)}
        for k, (i, val) in bad.items():
            T[k, i] = val
        mo = M.MultiOutputGP_GPU(X, T, nugget=1e-5, priors=weak(3, 1e-5))
        theta = np.tile(np.array([1., 1., 1., 0.]), (B, 1))
        t0 = timeouts()
        for _ in range(3):
            f, _, ok = mo._mogp_gpu.eval(theta, grad=False)
        assert timeouts() == t0, "non-finite targets were re-solved as chain time-outs"
        for k in range(B):
            if k in bad:
                assert not np.isfinite(f[k])
            else:
                assert ok[k] and np.isfinite(f[k])
        good = [k for k in range(B) if k not in bad][:2]
        for k in good:
            assert_allclose(f[k], R.GPRef(X, T[k], nugget=1e-5).fit(theta[k]), rtol=1e-8)      # (d = 3, unit length scales, nugget 1e-5: cond(K) ~ 1e8)


_STARTS_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd import libgpgpu
from test_gpu_parity import synth
X, T, _ = synth(4242, 300, 4, 6, 8)
# a multi-start fit of ANOTHER problem of the same shape first: the replica engine it leaves behind (Engine::fit_map keeps one per process,
# MOGP_REPLICA_CACHE) is taken again by the fit that is checked -- with other inputs, targets and priors in every slot
X0, T0, _ = synth(99, 300, 4, 6, 8)
libgpgpu.set_fit_options(max_iter=5, ftol=1e-9, gtol=1e-6, seed=3)
M.fit_GP_MAP(M.MultiOutputGP_GPU(X0, T0, nugget="fit"), n_tries=5)
libgpgpu.set_fit_options(max_iter=40, ftol=1e-9, gtol=1e-6, seed=11)
mo = M.fit_GP_MAP(M.MultiOutputGP_GPU(X, T, nugget="fit"), n_tries=5)
assert mo.get_indices_not_fit() == []
import ctypes
from mogp_emulator_amd import _capi
c = ctypes.c_longlong()
_capi.load().mogp_profile_counter(b"replica_engines_reused", ctypes.byref(c))
print("REUSED", c.value)
print("STARTS-OK", " ".join(repr(float(em.current_logpost)) for em in mo.emulators))
"""


def test_fit_GP_MAP_is_independent_of_how_the_starts_are_scheduled():
    """The starts of fit_GP_MAP run on replica engines, as many at a time as the replica cap allows (Engine::fit_map).  The
    starting points are drawn before the scheduling and a run never sees its batch neighbours, so all starts at once,
    capped passes (2 + 2 + 1 starts) and one start after the other must end at the same optima."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _STARTS_SCRIPT % {"root": root, "tests": os.path.join(root, "tests")}
    res, reused = [], []
    for env in ({}, {"MOGP_START_REPLICAS": "12"}, {"MOGP_PARALLEL_STARTS": "0"}, {"MOGP_LAZY_GRAD": "1"}, {"MOGP_REPLICA_CACHE": "0"}):
        out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "STARTS-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        res.append(np.array([float(x) for x in out.stdout.split("STARTS-OK")[1].split()]))
        reused.append(int(out.stdout.split("REUSED")[1].split()[0]))
    assert_allclose(res[1], res[0], rtol=1e-9)
    assert_allclose(res[2], res[0], rtol=1e-9)
    # round 6: the second fit of the process ran on the replica engine the first one left behind (same shape) -- and ends where a fit on a
    # fresh engine ends (MOGP_REPLICA_CACHE=0), bit for bit
    assert reused[0] == 1 and reused[1] == 1 and reused[2] == 0 and reused[4] == 0, reused
    assert np.array_equal(res[4], res[0])
    # gradient only for trial points that pass the sufficient-decrease test (the default from n = 512): the same decisions,
    # alpha by back substitution instead of the product with L^-1 -- the optima agree to the optimiser's tolerance
    assert_allclose(res[3], res[0], rtol=1e-6)


def test_c5_shaped_single_large_identities():
    # n = 4000, d = 8 (C5 family at a quarter size): no oracle, identities only
    n, d = 4000, 8
    X, T, Xs = synth(20240607 + 5, n, d, 1, 300)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
    eta = 1e-6
    gp = make_gp(X, T[0], nugget=eta)
    gp.fit(theta)
    a = gp.Kinv_t
    K = gp.get_K_matrix()
    assert np.abs(K @ a + eta * a - T[0]).max() < 1e-7
    tm, tv, _ = gp.predict(X[:128], deriv=False, include_nugget=False)
    assert_allclose(tm, T[0, :128] - eta * a[:128], rtol=1e-7, atol=1e-8)
    assert np.all(tv >= 0.) and np.all(tv < 2 * eta)
    L = gp.L
    assert_allclose(2 * np.log(np.diag(L)).sum(), np.linalg.slogdet(K + eta * np.eye(n))[1], rtol=1e-9)


def test_c4_shaped_matern_fit_nugget_identities():
    # C4 family: Matern-5/2 with fitted nugget, d = 20, several outputs, n = 3000 (ragged: NP = 3072)
    n, d, B = 3000, 20, 4
    X, T, Xs = synth(20240607 + 4, n, d, B, 300)
    eta = 1e-4
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0., np.log(eta)])
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget="fit", priors=weak(d, "fit"))
    f, g, ok = mo._mogp_gpu.eval(np.tile(theta, (B, 1)), grad=True)
    assert ok.all() and np.all(np.isfinite(g))
    mo.fit(np.tile(theta, (B, 1)))
    tm, tv, _ = mo.predict(X[:200], deriv=False, include_nugget=False)
    for k in range(B):
        em = mo.emulators[k]
        assert_allclose(em.nugget, eta, rtol=1e-14)
        a = em.Kinv_t
        assert_allclose(tm[k], T[k, :200] - eta * a[:200], rtol=1e-8, atol=1e-9)
        assert np.all(tv[k] >= 0.) and np.all(tv[k] <= eta * (1 + 1e-9))
    # finite-difference check of two gradient components at full size
    h = 1e-5
    for p in (0, d + 1):
        e = np.zeros_like(theta); e[p] = h
        fp, _, _ = mo._mogp_gpu.eval(np.tile(theta + e, (B, 1)), grad=False)
        fm, _, _ = mo._mogp_gpu.eval(np.tile(theta - e, (B, 1)), grad=False)
        assert_allclose(g[:, p], (fp - fm) / (2 * h), rtol=2e-5, atol=1e-4)


def test_c4_full_size_vs_oracle():
    # C4 at BASELINE size (n = 5000, d = 20, Matern-5/2, fitted nugget), two of the 16 outputs against the oracle with a
    # row-chunked distance build (the faithful (n, n, d) temporary would be 4 GB; per-entry arithmetic is unchanged)
    n, d, B = 5000, 20, 2
    X, T, Xs = synth(4, n, d, B, 200)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0., np.log(1e-4)])
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget="fit", priors=weak(d, "fit"))
    f, g, ok = mo._mogp_gpu.eval(np.tile(theta, (B, 1)), grad=True)
    assert ok.all()
    mo.fit(np.tile(theta, (B, 1)))
    mean, unc, _ = mo.predict(Xs, deriv=False)
    for k in range(B):
        ref = R.GPRef(X, T[k], kernel="Matern52", nugget="fit", chunk_rows=256)
        assert_allclose(f[k], ref.fit(theta), rtol=1e-10)
        rmu, rvar, _ = ref.predict(Xs)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-9)
        assert_allclose(unc[k], rvar, atol=1e-7)
        assert_allclose(mo.emulators[k].Kinv_t, ref.Kinv_t, rtol=1e-7, atol=1e-7 * np.abs(ref.Kinv_t).max())
        if k == 0:
            # the full gradient (20 length scales, sigma^2, fitted nugget) against the oracle's row-blocked gradient
            # (GaussianProcess.py:711-782; tests/test_oracle_golden.py pins the row-blocked form to the faithful one)
            gref = ref.logpost_deriv_chunked(theta, chunk_rows=256)
            assert_allclose(g[k], gref, rtol=1e-7, atol=1e-7 * np.abs(gref).max())


def test_c5_full_size_vs_oracle():
    # C5 at BASELINE size (one emulator, n = 16000, d = 8): log-posterior, gradient, K^-1 t and predictions against the
    # oracle (LAPACK dpotrf on the host, distance build and gradient in row chunks).
    # Tolerances scale with the conditioning: kappa_L = (max L_ii / min L_ii)^2 is a LOWER bound of
    # cond(K + eta I) (~1e6 here; the true condition number lies between it and n sigma^2 / eta ~ 1e10), and two
    # backward-stable factorisations of the same matrix (tools/chol128_probe.hip: max|L L^T - A| / max|A| = 1.3e-15 for the
    # device factor and for LAPACK's alike) differ by ~cond * eps in the quadratic form and in K^-1 t: observed 6 kappa_L eps
    # in the log-posterior, allowed 32 kappa_L eps (6e-9).  The variance keeps its absolute bar (1e-7 sigma^2), the mean
    # its rtol 1e-7.
    n, d = 16000, 8
    X, T, Xs = synth(5, n, d, 1, 64)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])
    gp = make_gp(X, T[0], "SquaredExponential", 1e-6)
    lp = gp.logposterior(theta)
    grad = gp.logpost_deriv(theta)
    gp.fit(theta)
    mean, unc, _ = gp.predict(Xs, deriv=False)
    ref = R.GPRef(X, T[0], nugget=1e-6, chunk_rows=128)
    lp_ref = ref.fit(theta)
    dl = np.diag(ref.L)
    kappa_eps = (dl.max() / dl.min()) ** 2 * np.finfo(float).eps
    assert 1e-10 < kappa_eps < 1e-6
    assert_allclose(lp, lp_ref, rtol=max(1e-10, 32 * kappa_eps))
    rmu, rvar, _ = ref.predict(Xs)
    assert_allclose(mean, rmu, rtol=1e-7, atol=1e-9)          # (atol as in the C4 test: the means are ~0.1 - 1)
    assert_allclose(unc, rvar, atol=1e-7)
    assert_allclose(gp.Kinv_t, ref.Kinv_t, rtol=1e-5, atol=1e-5 * np.abs(ref.Kinv_t).max())
    gref = ref.logpost_deriv_chunked(theta, chunk_rows=128)
    assert_allclose(grad, gref, rtol=1e-6, atol=max(1e-7, 64 * kappa_eps) * np.abs(gref).max())
    # Arbitration independent of LAPACK's arithmetic.  Each factor L stands for a matrix L L^T = K + E; the likelihood
    # of THAT matrix is computable in 80-bit long double from the factor in O(n^2) (oracle/exact.py).  Measured here, not argued:
    #  (i)   both factors are backward stable: ||(K - L L^T) v|| <= 1e-14 ||K|| ||v|| on random probes (products in long double);
    #  (ii)  each side's own fp64 solve + reductions reproduce the value of its factor to 1e-11 -- the arithmetic AFTER the factorisation
    #        is not where the two log-posteriors part;
    #  (iii) the two factors' exact values differ by what the conditioning allows, and the fp64 results differ by no more than that (+ (ii)):
    #        the 32 kappa_L eps bar above is the measured sensitivity of the likelihood to a backward-stable factor's error, with headroom.
    from oracle.exact import loglike_from_factor_longdouble, factor_backward_error
    L_dev = gp.L
    eta = 1e-6

    def K_rows(i0, i1):
        Kr = R.calc_K(R.calc_r2(X[i0:i1], X, theta[:d])) * np.exp(theta[d])
        Kr[np.arange(i1 - i0), np.arange(i0, i1)] += eta
        return Kr
    be_dev, be_ref = factor_backward_error(K_rows, L_dev, probes=2), factor_backward_error(K_rows, ref.L, probes=2)
    assert be_dev < 1e-14 and be_ref < 1e-14, (be_dev, be_ref)
    prior = lp_ref - 0.5 * (np.dot(ref.t, ref.Kinv_t) + R.logdet_L(ref.L) + n * np.log(2. * np.pi))
    ex_dev = float(loglike_from_factor_longdouble(L_dev, T[0]) + np.longdouble(prior))
    ex_ref = float(loglike_from_factor_longdouble(ref.L, T[0]) + np.longdouble(prior))
    assert abs(lp - ex_dev) <= 1e-11 * abs(ex_dev) and abs(lp_ref - ex_ref) <= 1e-11 * abs(ex_ref), (lp, ex_dev, lp_ref, ex_ref)
    gap = abs(ex_dev - ex_ref) / abs(ex_ref)
    assert gap <= 32 * kappa_eps and abs(lp - lp_ref) <= abs(ex_dev - ex_ref) + 2e-11 * abs(ex_ref), (gap, kappa_eps, lp, lp_ref)
    print("C5 arbitration: backward errors %.2e / %.2e, |fp64 - factor value| %.2e / %.2e, factor-to-factor %.2e = %.1f kappa_L eps" % (
        be_dev, be_ref, abs(lp - ex_dev) / abs(ex_dev), abs(lp_ref - ex_ref) / abs(ex_ref), gap, gap / kappa_eps))


def test_sharded_wrapper_on_one_gpu():
    # dist.ShardedMultiOutputGP with the real per-rank model (world size 1: no process group needed)
    from mogp_emulator_amd.dist import ShardedMultiOutputGP
    g = load_golden("mogp4.npz")
    D = g["X"].shape[1]
    sh = ShardedMultiOutputGP(g["X"], g["T"], nugget=1e-6, priors=weak(D, 1e-6))
    assert (sh.lo, sh.hi) == (0, 4)
    sh.fit(g["thetas"])
    res = sh.predict(g["Xs"])                      # the reference's surface: PredictResult(mean, unc, deriv), deriv=True by default
    mean, unc, der = res
    assert_allclose(mean, g["mean"], rtol=1e-7, atol=1e-9)
    assert_allclose(unc, g["var"], atol=1e-7)
    plain = M.MultiOutputGP_GPU(g["X"], g["T"], nugget=1e-6, priors=weak(D, 1e-6))
    plain.fit(g["thetas"])
    assert np.array_equal(der, plain.predict(g["Xs"]).deriv) and der.shape == (4, g["Xs"].shape[0], D)
    assert np.array_equal(sh(g["Xs"]), mean)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257, 383, 640])
def test_tile_boundary_sizes_vs_oracle(n):
    # n around the 64 / 128 tile edges (the y row sits at index n, padding starts at n+1)
    rng = np.random.default_rng(100 + n)
    D = 3
    X = rng.uniform(0, 1, (n, D))
    t = np.sin(X.sum(axis=1) * 3) + 0.1 * rng.normal(size=n)
    Xs = rng.uniform(0, 1, (37, D))
    theta = np.array([2.0, 1.5, 2.5, 0.3, np.log(1e-3)])
    for kern in KERNELS:
        gp = make_gp(X, t, kern, "fit")
        ref = R.GPRef(X, t, kernel=kern, nugget="fit")
        assert_allclose(gp.logposterior(theta), ref.fit(theta), rtol=1e-10, atol=1e-9)
        assert_allclose(gp.logpost_deriv(theta), ref.logpost_deriv(theta), rtol=1e-8, atol=1e-9)
        assert_allclose(gp.Kinv_t, ref.Kinv_t, rtol=1e-8, atol=1e-10)
        mean, unc, deriv = gp.predict(Xs)
        mu, var, rd = ref.predict(Xs, deriv=True)
        assert_allclose(mean, mu, rtol=1e-9, atol=1e-11)
        assert_allclose(unc, var, rtol=1e-8, atol=1e-10)
        assert_allclose(deriv, rd, rtol=1e-8, atol=1e-9)
        Q = np.zeros((n, n)); gp._densegp_gpu.get_invQ(Q)
        assert_allclose(Q @ (gp.get_K_matrix() + 1e-3 * np.eye(n)), np.eye(n), atol=1e-9)


# ----------------------------------------------------------------------------------------------------
# analytic mean function (CPU-class semantics, weak mean priors) on the device.
# fp64 tolerances: logpost rtol 1e-8, beta / K^-1(t - H beta) rtol 1e-6 (cond(K) ~ 1e9 at nugget 1e-5),
# gradient rtol/atol 1e-6, predictions rtol 1e-6.
# ----------------------------------------------------------------------------------------------------
MEAN_TERMS = {"lin": [(0, 1)], "two": [(0, 1), (2, 1)], "const": [], "quad": [(0, 1), (2, 2)]}


def native_mean(terms):
    return LibGPGPU.PolyMeanFunc(terms) if terms else LibGPGPU.ConstMeanFunc()


@pytest.mark.parametrize("tag", list(MEAN_TERMS))
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("mode", ["fixed", "fit"])
def test_analytic_mean_vs_reference_golden(tag, kern, mode):
    g = load_golden("meanfunc.npz")
    pre = "%s_%s_%s_" % (tag, kern, mode)
    nug = {"fixed": 1.e-5, "fit": "fit"}[mode]
    gp = make_gp(g["X"], g["t"], kern, nug, mean=native_mean(MEAN_TERMS[tag]), analytic_mean=True)   # weak priors, as the fixture
    theta = g[pre + "theta"]
    assert gp.n_params == theta.shape[0]               # mean coefficients are NOT part of theta in this mode
    # the value (~40) is a difference of O(1400) terms (quadratic form vs log det) at cond(K) ~ 1e9
    assert_allclose(gp.logposterior(theta), g[pre + "logpost"], rtol=1e-8)
    gp.fit(theta)
    assert_allclose(gp._densegp_gpu.get_beta(), g[pre + "beta"], rtol=1e-6, atol=1e-8)
    assert_allclose(gp.Kinv_t, g[pre + "Kinv_t_mean"], rtol=1e-6, atol=1e-6 * np.abs(g[pre + "Kinv_t_mean"]).max())
    assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-6, atol=1e-6)
    mu, var, _ = gp.predict(g["Xs"])
    assert_allclose(mu, g[pre + "mean"], rtol=1e-7, atol=1e-8)
    assert_allclose(var, g[pre + "var"], rtol=1e-6, atol=1e-9)


def test_analytic_mean_adaptive_nugget_vs_oracle(kern="Matern52"):
    # (squared exponential with zero jitter has cond(K) ~ 1/eps here: no meaningful reference value)
    g = load_golden("meanfunc.npz")
    theta = g["quad_%s_adaptive_theta" % kern]
    gp = make_gp(g["X"], g["t"], kern, "adaptive", mean=native_mean(MEAN_TERMS["quad"]), analytic_mean=True)
    gp.fit(theta)
    ref = R.GPRefMean(g["X"], g["t"], MEAN_TERMS["quad"], True, kernel=kern, nugget=float(gp.nugget))
    lp = ref.fit(theta)
    assert_allclose(gp.current_logpost, lp, rtol=1e-8)
    mu, var, _ = gp.predict(g["Xs"])
    rmu, rvar, _ = ref.predict(g["Xs"])
    assert_allclose(mu, rmu, rtol=1e-6, atol=1e-7)
    assert_allclose(var, rvar, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("n", [60, 126, 127, 128, 255, 300])
def test_analytic_mean_multioutput_tile_boundaries(n):
    # rows n .. n+q of the factorised matrix carry [t, H]: make them straddle 64- and 128-tile edges
    rng = np.random.default_rng(100 + n)
    d, n_out, m = 3, 5, 37
    X = rng.random((n, d))
    Xs = rng.random((m, d))
    T = np.stack([np.sin(3 * X[:, 0] + k) + (k + 1) * X[:, 2] ** 2 + 0.5 * k for k in range(n_out)])
    terms = MEAN_TERMS["quad"]
    mo = M.MultiOutputGP_GPU(X, T, mean=native_mean(terms), kernel="Matern52", nugget="fit", priors=weak(d, "fit"),
                             analytic_mean=True)
    thetas = np.stack([np.r_[rng.uniform(0., 2., d), rng.uniform(-1., 1.), rng.uniform(-9., -6.)] for _ in range(n_out)])
    f, grad, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    mo.fit(thetas)
    mean, unc, deriv = mo.predict(Xs)
    for k in range(n_out):
        ref = R.GPRefMean(X, T[k], terms, True, kernel="Matern52", nugget="fit")
        assert_allclose(f[k], ref.fit(thetas[k]), rtol=1e-9)
        assert_allclose(grad[k], ref.logpost_deriv(thetas[k]), rtol=1e-6, atol=1e-6)
        rmu, rvar, _ = ref.predict(Xs)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(unc[k], rvar, rtol=1e-6, atol=1e-9)
        assert_allclose(mo._mogp_gpu.emulator(k).get_beta(), ref.beta, rtol=1e-6, atol=1e-8)
    # d mean / d x* against central differences of the predictive mean itself
    h = 1e-6
    for dd in range(d):
        e = np.zeros(d)
        e[dd] = h
        fd = (mo.predict(Xs + e, unc=False, deriv=False)[0] - mo.predict(Xs - e, unc=False, deriv=False)[0]) / (2 * h)
        assert_allclose(deriv[:, :, dd], fd, rtol=1e-5, atol=1e-6)


def test_analytic_mean_fit_GP_MAP_and_limits():
    rng = np.random.default_rng(5)
    n, d, n_out = 80, 2, 3
    X = rng.random((n, d))
    T = np.stack([np.cos(4 * X[:, 0]) + 2. * k * X[:, 1] + k + 0.01 * rng.normal(size=n) for k in range(n_out)])
    # proper priors on the correlation lengths keep the optimum away from the flat directions
    pri = GPPriors(corr=[InvGammaPrior(3., 1.), InvGammaPrior(3., 1.)], nugget_type="fit")
    mo = M.MultiOutputGP_GPU(X, T, mean=native_mean([(1, 1)]), kernel="Matern52", nugget="fit", priors=pri, analytic_mean=True)
    theta0 = np.array([0., 0., 0., np.log(1e-3)])
    LibGPGPU.set_fit_options(max_iter=500, ftol=1e-12, gtol=1e-8, seed=3)
    mo = M.fit_GP_MAP(mo, n_tries=1, theta0=theta0)
    LibGPGPU.set_fit_options(max_iter=200, ftol=1e-9, gtol=1e-6, seed=0)
    assert len(mo.get_indices_fit()) == n_out
    for k, em in enumerate(mo.emulators):
        th = em.theta
        theta = th.get_data()
        assert th.get_mean().shape == (0,)
        rpri = R.GPPriorsRef(d, "fit", corr=[R.Prior("invgamma", 3., 1.), R.Prior("invgamma", 3., 1.)])
        ref = R.GPRefMean(X, T[k], [(1, 1)], True, kernel="Matern52", nugget="fit", priors=rpri)
        assert_allclose(em.current_logpost, ref.fit(theta), rtol=1e-7)
        # trajectory parity is unpinned: the end point must be at least as good as scipy's from the same start
        sci = R.fit_GP_MAP_ref(R.GPRefMean(X, T[k], [(1, 1)], True, kernel="Matern52", nugget="fit", priors=rpri),
                               n_tries=1, theta0=theta0)
        assert em.current_logpost <= sci.current_logpost + 1e-5 * abs(sci.current_logpost)
        # the slope on x[1] is recovered by the analytic coefficients
        assert_allclose(em._densegp_gpu.get_beta()[1], 2. * k, atol=0.75)
    # more than 7 terms is refused loudly rather than silently truncated
    with pytest.raises(RuntimeError, match="at most"):
        M.GaussianProcessGPU(X, T[0], mean=native_mean([(0, p) for p in range(1, 9)]), analytic_mean=True)
    # a parameter-free mean has nothing to integrate out: identical to the plain path
    a = M.GaussianProcessGPU(X, T[0], nugget=1e-6, analytic_mean=True)
    b = M.GaussianProcessGPU(X, T[0], nugget=1e-6)
    th = np.array([0.3, -0.2, 0.1])
    assert a.logposterior(th) == b.logposterior(th)


# ----------------------------------------------------------------------------------------------------
# predict(full_cov=True).  Tolerance: rtol 1e-6, atol 1e-7 * max|cov| (fp64, cond(K) ~ 1e9).
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["zero", "lin"])
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("mode", ["fixed", "fit"])
def test_full_cov_vs_reference_golden(tag, kern, mode):
    g = load_golden("fullcov.npz")
    pre = "%s_%s_%s_" % (tag, kern, mode)
    nug = {"fixed": 1.e-5, "fit": "fit"}[mode]
    kw = {} if tag == "zero" else dict(mean=native_mean([(1, 1)]), analytic_mean=True)
    gp = make_gp(g["X"], g["t"], kern, nug, **kw)
    gp.fit(g[pre + "theta"])
    scale = np.abs(g[pre + "cov"]).max()
    mu, cov, _ = gp.predict(g["Xs"], full_cov=True, deriv=False)
    assert cov.shape == (70, 70)
    assert_allclose(mu, g[pre + "mean"], rtol=1e-7, atol=1e-8)
    assert_allclose(cov, g[pre + "cov"], rtol=1e-6, atol=1e-7 * scale)
    assert_allclose(gp.predict(g["Xs"], full_cov=True, include_nugget=False)[1], g[pre + "cov_nonug"], rtol=1e-6, atol=1e-7 * scale)
    assert np.array_equal(cov, cov.T)                                  # mirrored, not recomputed
    assert_allclose(np.diag(cov), gp.predict(g["Xs"])[1], rtol=1e-6, atol=1e-7 * scale)


@pytest.mark.parametrize("m", [1, 127, 128, 129, 300])
def test_full_cov_multioutput_tile_boundaries(m):
    X, T, _ = synth(21, 333, 4, 3, 1)
    Xs = np.random.default_rng(m).random((m, 4))
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget="fit", priors=weak(4, "fit"))
    rng = np.random.default_rng(3)
    thetas = np.stack([np.r_[rng.uniform(0., 2., 4), rng.uniform(-1., 1.), rng.uniform(-9., -6.)] for _ in range(3)])
    mo.fit_emulator(0, thetas[0])
    mo.fit_emulator(2, thetas[2])                # emulator 1 stays unfit: NaN rows under allow_not_fit
    mean, cov, _ = mo.predict(Xs, full_cov=True, deriv=False, allow_not_fit=True)
    assert cov.shape == (3, m, m) and np.all(np.isnan(cov[1])) and np.all(np.isnan(mean[1]))
    for k in (0, 2):
        ref = R.GPRef(X, T[k], kernel="Matern52", nugget="fit")
        ref.fit(thetas[k])
        rmu, rcov, _ = ref.predict(Xs, full_cov=True)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(cov[k], rcov, rtol=1e-6, atol=1e-7 * np.abs(rcov).max())
        # positive semi-definite up to rounding
        assert np.linalg.eigvalsh(cov[k]).min() > -1e-8 * np.abs(rcov).max()


# ----------------------------------------------------------------------------------------------------
# consumers of the batched prediction, fused on the device.
# Tolerance: rtol 1e-6 on scores (ratio of an rtol-1e-7 mean difference and the root of an atol-1e-7 variance).
# ----------------------------------------------------------------------------------------------------
def _consumer_mogp(g):
    mo = M.MultiOutputGP_GPU(g["X"], g["T"], nugget=1.e-4, priors=weak(2, 1.e-4))
    mo.fit(g["thetas"])
    return mo


def test_history_matching_implausibility_vs_reference():
    g = load_golden("consumers.npz")
    mo = _consumer_mogp(g)
    obs = [g["obs"], g["obs_var"]]
    for rank in range(3):
        hm = M.HistoryMatching(gp=mo, obs=obs, coords=g["Xs"])
        assert_allclose(hm.get_implausibility(rank=rank), g["I_rank%d" % rank], rtol=1e-6)
        hm = M.HistoryMatching(gp=mo, obs=obs, coords=g["Xs"])
        assert_allclose(hm.get_implausibility(g["disc"], rank=rank), g["I_disc_rank%d" % rank], rtol=1e-6)
    hm = M.HistoryMatching(gp=mo, obs=obs, coords=g["Xs"], threshold=2.5)
    assert hm.get_NROY(0.05, rank=1) == list(g["NROY"])
    assert hm.get_RO(0.05, rank=1) == list(g["RO"])
    single = M.HistoryMatching(gp=mo.emulators[1], obs=[-0.2, 0.02], coords=g["Xs"])
    assert_allclose(single.get_implausibility(0.07), g["I_single"], rtol=1e-6)
    # the fused device score equals the host formula applied to the device predictions
    mean, unc, _ = mo.predict(g["Xs"], deriv=False)
    assert_allclose(hm.I, R.implausibility_ref(g["obs"], g["obs_var"], mean, unc, 0.05, 1), rtol=1e-9)
    # error behaviour of the reference class (tests/test_HistoryMatching.py:393-405, 316-361)
    with pytest.raises(AssertionError):
        hm.get_implausibility(-1.)
    with pytest.raises(AssertionError):
        hm.get_implausibility(rank=3)
    with pytest.raises(ValueError):
        M.HistoryMatching(gp=mo, coords=g["Xs"]).get_implausibility()
    with pytest.raises(ValueError):
        M.HistoryMatching(gp=mo, obs=obs, coords=g["Xs"], expectations=M.PredictResult(mean=mean, unc=unc, deriv=None)).get_implausibility()
    # explicit expectations: the NumPy path, literals of tests/test_HistoryMatching.py:363-426
    pr = M.PredictResult(mean=np.array([2., 10.]), unc=np.array([0., 0.]), deriv=None)
    assert_allclose(M.HistoryMatching(obs=[1., 1.], expectations=pr).get_implausibility(), [1., 9.])
    assert M.HistoryMatching(obs=[1., 1.], expectations=pr).get_NROY() == [0]
    pr2 = M.PredictResult(mean=np.array([[2., 10.], [4., 6.]]), unc=np.full((2, 2), 0.5), deriv=None)
    assert_allclose(M.HistoryMatching(obs=[[1., 5.], 0.5], expectations=pr2).get_implausibility(1.), [1. / np.sqrt(2.)] * 2)


def test_implausibility_sweep_chunks_and_means():
    # a sweep larger than one device chunk, a fixed mean function, and 20 outputs with a deep rank
    X, T, Xs = synth(31, 150, 3, 20, 5000)
    theta = np.array([1., 0.5, 0.2, 0.1])
    mo = M.MultiOutputGP_GPU(X, T, mean=LibGPGPU.FixedMeanFunc(0.25), nugget=1e-5, priors=weak(3, 1e-5))
    mo.fit(np.tile(theta, (20, 1)))
    z, zv, dc = np.linspace(-1, 1, 20), np.full(20, 0.01), np.linspace(0., 0.2, 20)
    mean, unc, _ = mo.predict(Xs, deriv=False)
    for rank in (0, 1, 7, 15):
        I = mo._mogp_gpu.implausibility(Xs, z, zv, dc, rank=rank)
        assert_allclose(I, R.implausibility_ref(z, zv, mean, unc, dc, rank), rtol=1e-9)
    with pytest.raises(RuntimeError, match="rank"):
        mo._mogp_gpu.implausibility(Xs, z, zv, dc, rank=16)
    # a mean function with fitted parameters is scored through predict + the host formula
    mc = M.MultiOutputGP_GPU(X, T[:2], mean=LibGPGPU.ConstMeanFunc(), nugget=1e-5, priors=weak(3, 1e-5))
    mc.fit(np.tile(np.r_[0.1, theta], (2, 1)))
    hm = M.HistoryMatching(gp=mc, obs=[z[:2], zv[:2]], coords=Xs[:64])
    m2, u2, _ = mc.predict(Xs[:64], deriv=False)
    assert_allclose(hm.get_implausibility(rank=0), R.implausibility_ref(z[:2], zv[:2], m2, u2, 0., 0), rtol=1e-12)


def test_mice_criterion_vs_reference():
    g = load_golden("consumers.npz")
    base = make_gp(g["X"], g["T"][0], nugget=1.e-4)
    base.fit(g["thetas"][0])
    cand = g["Xs"][:60]
    for s in (1, 10):
        crit, best = M.mice_criterion(base, cand, nugget_s=float(s))
        assert_allclose(crit, g["mice_crit_s%d" % s], rtol=1e-6)
        assert best == int(np.argmax(g["mice_crit_s%d" % s]))
    fast = M.MICEFastGP(cand, np.ones(60), nugget=1.e-4, priors=weak(2, 1.e-4))
    fast.fit(g["thetas"][0])
    assert_allclose(fast.loo_variance(), g["mice_unc2_s1"], rtol=1e-6)
    assert_allclose(fast.fast_predict(7), g["mice_unc2_s1"][7:8], rtol=1e-6)
    with pytest.raises(AssertionError):
        fast.fast_predict(60)
    # a larger candidate set against the leave-one-out identity evaluated by the oracle
    X, T, Xs = synth(32, 300, 4, 1, 700)
    theta = np.array([0.8, 1.1, 0.3, 0.6, 0.2])
    gp = make_gp(X, T[0], "Matern52", 1e-5)
    gp.fit(theta)
    crit, best = M.mice_criterion(gp, Xs, nugget_s=2.)
    ref = R.GPRef(X, T[0], kernel="Matern52", nugget=1e-5)
    ref.fit(theta)
    cg = R.GPRef(Xs, np.ones(700), kernel="Matern52", nugget=2e-5)
    cg.fit(theta)
    expected = ref.predict(Xs)[1] * np.diag(R.cho_solve_L(cg.L, np.eye(700)))
    assert_allclose(crit, expected, rtol=1e-5)
    assert best == int(np.argmax(expected))


# ----------------------------------------------------------------------------------------------------
# the reference's CPU-only kernels on the device.  Same fp64 tolerances as the stationary kernels.
# ----------------------------------------------------------------------------------------------------
CPU_ONLY_KERNELS = {"UniformSqExp": 1, "UniformMat52": 1, "ProductMat52": 3}


@pytest.mark.parametrize("name", list(CPU_ONLY_KERNELS))
@pytest.mark.parametrize("mode", ["fixed", "fit"])
def test_cpu_only_kernels_vs_reference_golden(name, mode):
    g = load_golden("kernels_cpuonly.npz")
    pre = "%s_%s_" % (name, mode)
    nc = CPU_ONLY_KERNELS[name]
    nug = {"fixed": 1.e-5, "fit": "fit"}[mode]
    gp = M.GaussianProcessGPU(g["X"], g["t"], kernel=name, nugget=nug, priors=GPPriors(n_corr=nc, nugget_type=mode))
    theta = g[pre + "theta"]
    assert gp.n_corr == nc and gp.n_params == theta.shape[0]
    assert_allclose(gp.logposterior(theta), g[pre + "logpost"], rtol=1e-9)
    assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-6, atol=1e-6)
    assert_allclose(gp.Kinv_t, g[pre + "Kinv_t"], rtol=1e-6, atol=1e-6 * np.abs(g[pre + "Kinv_t"]).max())
    mu, var, deriv = gp.predict(g["Xs"])
    assert_allclose(mu, g[pre + "mean"], rtol=1e-7, atol=1e-8)
    assert_allclose(var, g[pre + "var"], rtol=1e-6, atol=1e-9)
    # get_K: sigma^2 k(X, X) without nugget, against the reference's kernel_f restated by the oracle
    K = gp.get_K_matrix()
    assert_allclose(K, np.exp(theta[nc]) * R.kernel_f(g["X"], g["X"], theta[:nc], name), rtol=1e-12, atol=1e-15)
    # d mean / d x* against the oracle's analytic input derivative
    ref = R.GPRef(g["X"], g["t"], kernel=name, nugget=nug)
    ref.fit(theta)
    assert_allclose(deriv, ref.predict(g["Xs"], deriv=True)[2], rtol=1e-6, atol=1e-7)
    if mode == "fit":
        # default priors: one InvGamma per correlation parameter (the uniform kernels pool all inputs)
        gd = M.GaussianProcessGPU(g["X"], g["t"], kernel=name, nugget="fit")
        assert_allclose(gd.logposterior(theta), g[name + "_defprior_logpost"], rtol=1e-8)
        assert_allclose(gd.logpost_deriv(theta), g[name + "_defprior_grad"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("name", list(CPU_ONLY_KERNELS))
def test_cpu_only_kernels_multioutput_fit_and_full_cov(name):
    nc = CPU_ONLY_KERNELS[name]
    X, T, Xs = synth(41, 260, 3, 4, 90)
    mo = M.MultiOutputGP_GPU(X, T, kernel=name, nugget="fit", priors=GPPriors(n_corr=nc, nugget_type="fit"))
    assert mo.n_corr == [nc] * 4 and mo.n_params == [nc + 2] * 4
    rng = np.random.default_rng(2)
    thetas = np.stack([np.r_[rng.uniform(0., 2., nc), rng.uniform(-1., 1.), rng.uniform(-9., -6.)] for _ in range(4)])
    f, grad, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    mo.fit(thetas)
    mean, cov, _ = mo.predict(Xs, full_cov=True, deriv=False)
    for k in range(4):
        ref = R.GPRef(X, T[k], kernel=name, nugget="fit")
        assert_allclose(f[k], ref.fit(thetas[k]), rtol=1e-9)
        assert_allclose(grad[k], ref.logpost_deriv(thetas[k]), rtol=1e-6, atol=1e-6)
        rmu, rcov, _ = ref.predict(Xs, full_cov=True)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(cov[k], rcov, rtol=1e-6, atol=1e-7 * np.abs(rcov).max())
    # the optimiser runs on the reduced parameter vector
    LibGPGPU.set_fit_options(seed=5)
    mo = M.fit_GP_MAP(mo, n_tries=1, theta0=np.r_[np.zeros(nc), 0., np.log(1e-4)])
    LibGPGPU.set_fit_options(seed=0)
    assert mo.get_indices_not_fit() == []
    f1 = np.array([em.current_logpost for em in mo.emulators])
    f0, _, _ = M.MultiOutputGP_GPU(X, T, kernel=name, nugget="fit", priors=GPPriors(n_corr=nc, nugget_type="fit"))._mogp_gpu.eval(
        np.tile(np.r_[np.zeros(nc), 0., np.log(1e-4)], (4, 1)), grad=False)
    assert np.all(f1 < f0)


def test_input_dimension_limits():
    # D up to 80 runs (LDS-staged coordinate tiles); beyond that the constructor refuses with a clear message
    rng = np.random.default_rng(80)
    n, m, D = 200, 30, 80
    X, Xs = rng.random((n, D)), rng.random((m, D))
    t = np.sin(X.sum(1))
    theta = np.r_[np.full(D, -2 * np.log(0.3 * np.sqrt(D))), 0.1]
    gp = make_gp(X, t, "Matern52", 1e-6)
    ref = R.GPRef(X, t, kernel="Matern52", nugget=1e-6)
    assert_allclose(gp.logposterior(theta), ref.fit(theta), rtol=1e-10)
    assert_allclose(gp.logpost_deriv(theta), ref.logpost_deriv(theta), rtol=1e-7, atol=1e-8)
    mu, var, dv = gp.predict(Xs)
    rmu, rvar, rd = ref.predict(Xs, deriv=True)
    assert_allclose(mu, rmu, rtol=1e-7, atol=1e-9)
    assert_allclose(var, rvar, atol=1e-7 * np.exp(0.1))
    assert_allclose(dv, rd, rtol=1e-6, atol=1e-8)
    with pytest.raises(RuntimeError, match="input dimensions"):
        M.GaussianProcessGPU(rng.random((50, 81)), rng.random(50))


def test_c_abi_from_plain_c(tmp_path):
    # the drop-in boundary is usable from C with nothing but include/mogp_hip.h and the shared library
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "abi_roundtrip")
    libdir = os.path.join(root, "mogp_emulator_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "c", "abi_roundtrip.c"), "-o", exe, "-L" + libdir, "-lmogp_hip",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    vals = {line.split()[0]: line.split()[1:] for line in out.strip().splitlines()}
    # known answers of the reference's 2 x 3 fixture (tests/test_GaussianProcess.py:556-585)
    assert_allclose(float(vals["logpost"][0]), 6.516671478123768, rtol=1e-12)
    assert_allclose([float(v) for v in vals["alpha"]], [0.7357588823428844, 1.471517764685769], rtol=1e-12)
    assert_allclose(float(vals["grad3"][0]), -2.6787944117144216, rtol=1e-10)
    assert_allclose(float(vals["mean"][0]), 0.03390252374096476, rtol=1e-10)
    assert_allclose(float(vals["var"][0]), 2.717500758226203, rtol=1e-10)
    assert "Shape of new GPParams object does not match existing one" in out


# ----------------------------------------------------------------------------------------------------
# Analytic mean with informative mean priors: MeanPriors(mean = b, cov = scalar / vector / matrix), Priors.py:423-581.
# ----------------------------------------------------------------------------------------------------
MEANPRIOR_TERMS = {"scalar": [(0, 1)], "vector": [(0, 1), (2, 2)], "matrix": [(0, 1), (2, 2)], "tight": []}


@pytest.mark.parametrize("tag", list(MEANPRIOR_TERMS))
@pytest.mark.parametrize("kern", KERNELS)
@pytest.mark.parametrize("mode", ["fixed", "fit"])
def test_informative_mean_priors_vs_reference_golden(tag, kern, mode):
    from mogp_emulator_amd.Priors import MeanPriors
    g = load_golden("meanpriors.npz")
    pre = "%s_%s_%s_" % (tag, kern, mode)
    nug = {"fixed": 1.e-5, "fit": "fit"}[mode]
    pri = GPPriors(mean=MeanPriors(mean=g[pre + "b"], cov=g[pre + "cov"]), n_corr=3, nugget_type=mode)
    gp = M.GaussianProcessGPU(g["X"], g["t"], mean=native_mean(MEANPRIOR_TERMS[tag]), kernel=kern, nugget=nug, priors=pri,
                              analytic_mean=True)
    theta = g[pre + "theta"]
    assert_allclose(gp.logposterior(theta), g[pre + "logpost"], rtol=1e-8)
    gp.fit(theta)
    assert_allclose(gp._densegp_gpu.get_beta(), g[pre + "beta"], rtol=1e-6, atol=1e-8)
    assert_allclose(gp.Kinv_t, g[pre + "Kinv_t_mean"], rtol=1e-6, atol=1e-6 * np.abs(g[pre + "Kinv_t_mean"]).max())
    assert_allclose(gp.logpost_deriv(theta), g[pre + "grad"], rtol=1e-6, atol=1e-6)
    mu, var, _ = gp.predict(g["Xs"])
    assert_allclose(mu, g[pre + "mean"], rtol=1e-7, atol=1e-8)
    assert_allclose(var, g[pre + "var"], rtol=1e-6, atol=1e-9)
    cov = gp.predict(g["Xs"], full_cov=True, deriv=False)[1]
    assert_allclose(cov, g[pre + "cov_full"], rtol=1e-6, atol=1e-7 * np.abs(g[pre + "cov_full"]).max())


def test_mean_priors_per_emulator_and_errors():
    from mogp_emulator_amd.Priors import MeanPriors
    rng = np.random.default_rng(9)
    n, d = 140, 3
    X = rng.random((n, d))
    T = np.stack([np.sin(3 * X[:, 0]) + (k + 1) * X[:, 1] + 0.5 * k for k in range(3)])
    Xs = rng.random((25, d))
    terms = [(1, 1)]
    mps = [None, ([0.2, 1.0], 2.0), ([1.0, 3.0], [[1.0, 0.2], [0.2, 0.5]])]
    priors = [GPPriors(mean=mp, n_corr=d, nugget_type="fit") for mp in mps]
    mo = M.MultiOutputGP_GPU(X, T, mean=native_mean(terms), kernel="Matern52", nugget="fit", priors=priors, analytic_mean=True)
    thetas = np.stack([np.r_[rng.uniform(0., 2., d), rng.uniform(-1., 1.), rng.uniform(-9., -6.)] for _ in range(3)])
    f, grad, ok = mo._mogp_gpu.eval(thetas, grad=True)
    mo.fit(thetas)
    mean, unc, _ = mo.predict(Xs, deriv=False)
    for k in range(3):
        ref = R.GPRefMean(X, T[k], terms, True, mean_prior=mps[k], kernel="Matern52", nugget="fit")
        assert_allclose(f[k], ref.fit(thetas[k]), rtol=1e-9)
        assert_allclose(grad[k], ref.logpost_deriv(thetas[k]), rtol=1e-6, atol=1e-6)
        rmu, rvar, _ = ref.predict(Xs)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(unc[k], rvar, rtol=1e-6, atol=1e-9)
    # mean priors without the analytic mean, or with the wrong length, are refused
    with pytest.raises(NotImplementedError):
        M.GaussianProcessGPU(X, T[0], mean=native_mean(terms), priors=GPPriors(mean=mps[1], n_corr=d, nugget_type="adaptive"))
    with pytest.raises(RuntimeError, match="one entry per mean-function term"):
        M.GaussianProcessGPU(X, T[0], mean=native_mean(terms), priors=GPPriors(mean=([1., 2., 3.], 1.0), n_corr=d, nugget_type="adaptive"),
                             analytic_mean=True)
    with pytest.raises(ValueError):
        MeanPriors(mean=[1., 2.])
    with pytest.raises(AssertionError):
        MeanPriors(mean=[1., 2.], cov=-1.)


# ------------------------------------------------------------------------------------------------
# stand-alone kernel objects and MeanPriors of the native module (bindings.cu:340-361, 558-582)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, cls", [("SquaredExponential", "SquaredExponentialKernel"), ("Matern52", "Matern52Kernel")])
def test_kernel_objects_vs_reference_golden(name, cls):
    """kernel_f / kernel_deriv for x1 != x2 against the arrays the reference's Kernel.kernel_f / kernel_deriv produced
    (tests/golden/kernels.npz, Kernel.py:99-173); the native objects carry log sigma^2 as their last parameter."""
    from mogp_emulator_amd import libgpgpu
    g = load_golden("kernels.npz")
    x1, x2, theta = g["x1"], g["x2"], g["theta"]
    kern = getattr(libgpgpu, cls)()
    logs2 = 0.7
    params = np.concatenate([theta, [logs2]])
    s2 = np.exp(logs2)
    K = kern.kernel_f(x1, x2, params)
    assert K.shape == (7, 5)
    assert_allclose(K, s2 * g[name + "_K"], rtol=1e-13)
    dK = kern.kernel_deriv(x1, x2, params)
    assert dK.shape == (4 * 7 * 5,)
    dK = dK.reshape(4, 7, 5)
    assert_allclose(dK[:3], s2 * g[name + "_dKdtheta"], rtol=1e-12, atol=1e-15)
    assert_allclose(dK[3], K, rtol=1e-14)
    # input derivatives: flat (n2, n1, D) order of the reference's CUDA kernel, checked by central differences of kernel_f
    dX = kern.kernel_inputderiv(x1, x2, params)
    assert dX.shape == (5 * 7 * 3,)
    dX = dX.reshape(5, 7, 3)
    h = 1e-6
    for d in range(3):
        e = np.zeros(3); e[d] = h
        fd = (kern.kernel_f(x1 + e, x2, params) - kern.kernel_f(x1 - e, x2, params)) / (2 * h)
        assert_allclose(dX[:, :, d].T, fd, rtol=1e-6, atol=1e-8)
    # the oracle's analytic input derivative (what predict_deriv is checked against) has the CPU (D, n1, n2) order
    assert_allclose(np.transpose(dX, (2, 1, 0)), s2 * R.kernel_inputderiv(x1, x2, theta, name), rtol=1e-11, atol=1e-14)
    # closed forms of tests/test_Kernel.py:8-38
    Kc = kern.kernel_f(g["closed_x"], g["closed_y"], np.array([0., 0.]))
    assert_allclose(Kc, g[name + "_closed_K"], rtol=1e-14)
    assert kern.get_n_params(x1) == 3
    with pytest.raises(RuntimeError):
        kern.kernel_f(x1, x2, theta)                   # one parameter short (no log sigma^2)
    with pytest.raises(RuntimeError):
        kern.kernel_f(x1, x2[:, :2], params)


@pytest.mark.parametrize("name, cls", [("UniformSqExp", "UniformSqExpKernel"), ("UniformMat52", "UniformMat52Kernel"),
                                       ("ProductMat52", "ProductMat52Kernel")])
def test_cpu_only_kernel_objects_vs_reference_golden(name, cls):
    from mogp_emulator_amd import libgpgpu
    g = load_golden("kernels_cpuonly.npz")
    x1, x2 = g["X"][:7], g["Xs"][:5]                    # the point sets and parameters tests/golden/make_golden.py used
    kern = getattr(libgpgpu, cls)()
    nc = 1 if name.startswith("Uniform") else 3
    theta = np.array([0.7, -0.3, 1.1])[:nc]
    params = np.concatenate([theta, [0.]])
    assert_allclose(kern.kernel_f(x1, x2, params), g[name + "_kf"], rtol=1e-12)
    dK = kern.kernel_deriv(x1, x2, params).reshape(nc + 1, 7, 5)
    assert_allclose(dK[:nc], g[name + "_kd"], rtol=1e-11, atol=1e-14)


def test_native_meanpriors_object():
    """LibGPGPU.MeanPriors(mean, cov) with the accessor names of bindings.cu:558-582, usable for an analytic-mean emulator."""
    from mogp_emulator_amd import libgpgpu
    b = np.array([1.0, -0.5]); C = np.array([[2.0, 0.3], [0.3, 1.5]])
    mp = LibGPGPU.MeanPriors(b, C)
    assert mp.get_n_params() == 2 and not mp.has_weak_priors()
    assert_allclose(mp.get_mean(), b); assert_allclose(mp.get_cov(), C)
    assert_allclose(mp.inv_cov() @ C, np.eye(2), atol=1e-14)
    assert_allclose(mp.inv_cov_b(), np.linalg.solve(C, b)); assert_allclose(mp.logdet_cov(), np.log(np.linalg.det(C)))
    assert_allclose(mp.dm_dot_b(np.array([[1., 2.], [3., 4.]])), [0., 1.])
    assert libgpgpu.MeanPriors().has_weak_priors() and libgpgpu.MeanPriors().get_n_params() == 0
    # it drives the device the same way as the host-side Priors.MeanPriors value object
    from mogp_emulator_amd.Priors import MeanPriors as HostMeanPriors
    X, T, Xs = synth(3, 80, 2, 1, 6)
    t = T[0] + 2.0 + X[:, 0]
    gp_a = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", analytic_mean=True, nugget=1e-6,
                                priors=GPPriors(mean=HostMeanPriors(b, C), n_corr=2, nugget_type="fixed"))
    gp_b = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", analytic_mean=True, nugget=1e-6, priors=GPPriors(n_corr=2, nugget_type="fixed"))
    gp_b._densegp_gpu.set_mean_priors(*mp.native_params())
    th = np.array([0.3, 0.1, 0.2])
    assert gp_a.logposterior(th) == gp_b.logposterior(th)


def test_state_changes_invalidate_cached_results():
    """A new fixed nugget invalidates factor / alpha / log-posterior (refit required), new priors invalidate the cached
    log-posterior (the reference serves the stale values in both cases)."""
    X, T, Xs = synth(21, 90, 2, 1, 7)
    th = np.array([0.4, 0.2, 0.1])
    gp = M.GaussianProcessGPU(X, T[0], nugget=1e-6, priors=GPPriors(n_corr=2, nugget_type="fixed"))
    gp.fit(th)
    lp_small = gp.logposterior(th)
    gp.nugget = 1e-2
    assert not gp.theta.data_has_been_set()
    with pytest.raises(ValueError):
        gp.predict(Xs)
    lp_big = gp.logposterior(th)                      # refits with the new nugget
    ref = R.GPRef(X, T[0], nugget=1e-2)
    assert_allclose(lp_big, ref.fit(th), rtol=1e-10)
    assert abs(lp_big - lp_small) > 1.0
    mu, var, _ = ref.predict(Xs)
    assert_allclose(gp.predict(Xs).unc, var, atol=1e-9)
    # priors changed after a fit: same theta, the log-posterior is recomputed with the new priors
    gp._set_priors(GPPriors(corr=[InvGammaPrior(2., 1.), InvGammaPrior(2., 1.)], cov=InvGammaPrior(3., 2.), nugget_type="fixed"))
    pri = R.GPPriorsRef(2, "fixed", corr=[R.Prior("invgamma", 2., 1.)] * 2, cov=R.Prior("invgamma", 3., 2.))
    assert_allclose(gp.logposterior(th), R.GPRef(X, T[0], nugget=1e-2, priors=pri).fit(th), rtol=1e-10)
