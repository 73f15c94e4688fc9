"""Mixture prediction over hyperparameter samples on the MI355X (mogp_emulator_amd.predict_marginal, DenseGP_GPU / MultiOutputGP_GPU
.predict_mixture, csrc/kernels_mixture.hip) against the NumPy restatement (marginal_restate.py), at the smallest shapes where the code can go
wrong: n = 7 (one tile) and 130 (just past the 128 padding), D = 1 and 3, m = 1 and 37, S = 1, 5 and 33.

Tolerance.  Not fixed in advance: for every case the restatement is evaluated in float64 and in np.longdouble on the CPU, and the device is
allowed 100 x their disagreement -- relative to max|mean|, max within, the largest d_s^2 (long double) for `between`, and absolute for the
log-weights.  A disagreement below the spacing of float64 cannot be told from none (the long double result is compared with a float64 one),
so it counts as one spacing, 2^-52.  A case whose disagreement exceeds 1e-8 would be too ill-conditioned to judge a kernel with; every case
asserts that it is not.  Measured disagreements (this file prints them), hence bars: see DESIGN.md section 4.
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import hessian_restate as hr
import marginal_restate as mr

pytestmark = pytest.mark.gpu
MARGIN = 100.
ILL = 1e-8
EPS = 2. ** -52
LD = np.longdouble


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _data(n, D, m, seed=11, repeats=0):
    rng = np.random.default_rng(seed + 1000 * n + D)
    X = rng.random((n, D))
    if repeats:
        X[n - repeats:] = X[:repeats]
    t = np.sin(3 * X[:, 0]) + (X[:, 1] ** 2 if D > 1 else 0.)
    if not repeats:
        t = t + .1 * rng.standard_normal(n)
    return X, t, rng.random((m, D))


def _nc(kernel, D):
    return 1 if kernel in mr.UNIFORM else D


def _thetas(S, kernel, D, fit, const, seed=3, spread=0.15):
    """S samples around correlation lengths of 0.1 - 0.6 times sqrt(D) (test_gpu_hessian._theta): the matrices stay well conditioned"""
    nc = _nc(kernel, D)
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, nc) if nc > 1 else np.array([np.log(1. / D) + 2.5])
    base = np.concatenate([[0.2] if const else [], corr, [0.2], [-4.] if fit else []])
    return base + spread * np.random.default_rng(seed).standard_normal((S, base.size))


def _mean_arg(mean):
    if mean == "const":
        return LibGPGPU.ConstMeanFunc()
    if mean == "zero":
        return None
    return LibGPGPU.FixedMeanFunc(mean[1])


def _nugget_kind(nugget):
    return "fixed" if isinstance(nugget, float) else nugget


def _gp(X, t, kernel, nugget, mean="zero"):
    return M.GaussianProcessGPU(X, t, mean=_mean_arg(mean), kernel=kernel, nugget=nugget,
                                priors=GPPriors(n_corr=_nc(kernel, X.shape[1]), nugget_type=_nugget_kind(nugget)))


def _weights(kind, S):
    if kind == "uniform":
        return np.ones(S)
    w = 0.2 + 3. * np.random.default_rng(S).random(S)
    if S > 1:
        w[1] = 0.                                    # one exact zero
    return w


def _disagreement(a, b, what):
    """float64 restatement a against long double b: (relative disagreements, bars of the device in absolute terms)"""
    scale = {"mean": float(np.abs(b["mean"]).max()), "within": float(b["within"].max()), "between": float(b["d2max"])}
    dis, bars = {}, {}
    for k, sc in scale.items():
        d = float(np.abs(a[k] - b[k]).max())
        dis[k] = d / sc if sc > 0 else 0.
        assert dis[k] <= ILL, "the case is too ill-conditioned to test a kernel with (%s: %.3g)" % (k, dis[k])
        bars[k] = MARGIN * max(dis[k], EPS) * sc
    pos = b["weights"] > 0
    dis["logw"] = float(np.abs(np.log(a["weights"][pos]) - np.log(b["weights"][pos]).astype(float)).max()) if pos.any() else 0.
    assert dis["logw"] <= ILL
    bars["logw"] = MARGIN * max(dis["logw"], EPS)
    print("%s: float64 vs long double: mean %.3g of %.4g, within %.3g of %.4g, between %.3g of %.4g, log-weights %.3g" % (
        what, dis["mean"], scale["mean"], dis["within"], scale["within"], dis["between"], scale["between"], dis["logw"]))
    return dis, bars


def _reference(X, t, thetas, Xs, kernel, mean, fit, nuggets, weights, log_q, include_nugget, what):
    a = mr.mixture(X, t, thetas, Xs, kernel, mean, fit, nuggets, weights, log_q, include_nugget)
    b = mr.mixture(X, t, thetas, Xs, kernel, mean, fit, nuggets, weights, log_q, include_nugget, dtype=LD)
    assert np.array_equal(a["ok"], b["ok"])
    _, bars = _disagreement(a, b, what)
    return a, bars


def _close(got, ref, bars, what):
    mean, within, between, w = got[:4]
    for name, arr in (("mean", mean), ("within", within), ("between", between)):
        err = float(np.abs(arr - ref[name]).max())
        print("%s: device vs float64 restatement, %s %.3g (bar %.3g)" % (what, name, err, bars[name]))
        assert np.all(np.isfinite(arr))
        assert err <= bars[name], (what, name, err, bars[name])
    pos = ref["weights"] > 0
    assert np.array_equal(w > 0, pos), "the zero weights are exactly zero, the others are not"
    err = float(np.abs(np.log(w[pos]) - np.log(ref["weights"][pos])).max())
    print("%s: log-weights %.3g (bar %.3g)" % (what, err, bars["logw"]))
    assert err <= bars["logw"]
    assert abs(w.sum() - 1.) < 1e-14


# (n, D, m, S, kernel, nugget, mean, weights, include_nugget)
PARITY = [
    (7, 1, 1, 1, "SquaredExponential", 1e-4, "zero", "uniform", True),
    (7, 3, 37, 5, "Matern52", "fit", "zero", "nonuniform", True),
    (130, 3, 37, 5, "SquaredExponential", 1e-4, "zero", "nonuniform", False),
    (130, 1, 37, 33, "Matern52", 1e-4, "zero", "uniform", True),
    (130, 3, 1, 33, "UniformSqExp", "fit", "zero", "nonuniform", True),
    (7, 3, 37, 5, "UniformMat52", 1e-4, "const", "uniform", True),
    (130, 3, 37, 5, "Matern52", "fit", "const", "nonuniform", False),
    (130, 3, 37, 5, "Matern52", "adaptive", "zero", "uniform", True),
    (7, 1, 37, 33, "SquaredExponential", 1e-4, ("fixed", 0.3), "nonuniform", True),
]


@functools.lru_cache(maxsize=None)
def _parity_case(n, D, m, S, kernel, nugget, mean, wkind, include_nugget):
    X, t, Xs = _data(n, D, m)
    fit = nugget == "fit"
    thetas = _thetas(S, kernel, D, fit, mean == "const")
    w = _weights(wkind, S)
    # (a well-conditioned matrix factorises without jitter: the adaptive nugget of these samples is 0)
    nug = None if fit else (0. if nugget == "adaptive" else nugget)
    ref, bars = _reference(X, t, thetas, Xs, kernel, mean, fit, nug, w, None, include_nugget,
                           "n=%d D=%d m=%d S=%d %s %s %s" % (n, D, m, S, kernel, nugget, mean))
    return X, t, Xs, thetas, w, ref, bars


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "n%d-D%d-m%d-S%d-%s-%s-%s-%s-%s" % (c[:5] + (c[5], c[6] if isinstance(c[6], str) else "fixedmean", c[7], "nug" if c[8] else "nonug")))
def test_device_matches_restatement(case):
    n, D, m, S, kernel, nugget, mean, wkind, include_nugget = case
    X, t, Xs, thetas, w, ref, bars = _parity_case(*case)
    gp = _gp(X, t, kernel, nugget, mean)
    gp.fit(thetas[0])
    got = gp._densegp_gpu.predict_mixture(thetas, Xs, weights=w, include_nugget=include_nugget)
    assert got[0].shape == (m,) and got[3].shape == (S,) and got[5].all()
    _close(got, ref, bars, "parity")
    err = float(np.abs(got[4] - ref["F"]).max() / np.abs(ref["F"]).max())
    print("logpost: %.3g relative" % err)
    assert err <= 1e-9
    res = M.predict_marginal(gp, Xs, thetas=thetas, weights=w, include_nugget=include_nugget)
    for a, b in zip((res.mean, res.within, res.between, res.weights, res.logpost, res.ok), got):
        assert np.array_equal(a, b)                                            # two calls: the same bits
    assert np.array_equal(res.unc, res.within + res.between) and res.laplace_ok is None
    assert abs(res.ess - 1. / np.sum(ref["weights"] ** 2)) <= 1e-9 * S


@pytest.mark.parametrize("n,D,m,kernel,nugget,mean", [(7, 1, 1, "SquaredExponential", 1e-4, "zero"), (130, 3, 37, "Matern52", "fit", "const"),
                                                      (130, 3, 37, "UniformSqExp", "adaptive", "zero")])
@pytest.mark.parametrize("include_nugget", [True, False])
def test_one_sample_is_predict(n, D, m, kernel, nugget, mean, include_nugget):
    X, t, Xs = _data(n, D, m)
    theta = _thetas(1, kernel, D, nugget == "fit", mean == "const")
    gp = _gp(X, t, kernel, nugget, mean)
    gp.fit(theta[0])
    p = gp.predict(Xs, deriv=False, include_nugget=include_nugget)
    mean_, within, between, w, F, ok = gp._densegp_gpu.predict_mixture(theta, Xs, weights=np.array([1.]), include_nugget=include_nugget)
    assert_array_equal(mean_, p.mean)
    assert_array_equal(within, p.unc)
    assert not between.any() and w[0] == 1. and ok[0]
    assert F[0] == gp.logposterior(theta[0])


def _multi(E, n=130, D=3, m=37, S=5, kernel="Matern52", nugget=1e-4, devices=None):
    X, _, Xs = _data(n, D, m)
    rng = np.random.default_rng(9)
    T = np.array([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 + .1 * rng.standard_normal(n) for k in range(E)])
    mo = M.MultiOutputGP_GPU(X, T, kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_nugget_kind(nugget)), devices=devices)
    thetas = np.array([_thetas(S, kernel, D, nugget == "fit", False, seed=20 + e) for e in range(E)])
    w = np.array([_weights("nonuniform", S) + e for e in range(E)])
    return X, T, Xs, mo, thetas, w


def test_grouping_and_chunking_do_not_change_a_bit():
    X, T, Xs, mo, thetas, w = _multi(3)
    mo.fit(thetas[:, 0])
    lib = mo._mogp_gpu
    first = base = lib.predict_mixture(thetas, Xs, weights=w)
    assert np.all(np.isfinite(first[0])) and first[6].all() and first[2].max() > 0
    for a, b in zip(first, lib.predict_mixture(thetas, Xs, weights=w)):
        assert np.array_equal(a, b)
    for max_slots in (0, 1, 2, 5, 7):
        for max_points in (0, 1, 16):
            got = lib.predict_mixture(thetas, Xs, weights=w, max_slots=max_slots, max_points=max_points)
            for a, b in zip(first, got):
                assert np.array_equal(a, b), (max_slots, max_points)
    # and the same with importance weights, whose normalisation needs every sample of an emulator before the first pass
    q = np.random.default_rng(1).standard_normal(w.shape)
    first = lib.predict_mixture(thetas, Xs, log_q=q)
    for max_slots, max_points in ((2, 16), (7, 1)):
        for a, b in zip(first, lib.predict_mixture(thetas, Xs, log_q=q, max_slots=max_slots, max_points=max_points)):
            assert np.array_equal(a, b)
    ref, bars = _reference(X, T[2], thetas[2], Xs, "Matern52", "zero", False, 1e-4, w[2], None, True, "emulator 2 of 3")
    _close([a[2] for a in base[:4]], ref, bars, "emulator 2 of 3")


def test_the_fitted_state_survives():
    X, t, Xs = _data(130, 3, 37)
    thetas = _thetas(5, "Matern52", 3, True, False)
    gp = _gp(X, t, "Matern52", "fit")
    hat = thetas[0] + 0.05
    gp.fit(hat)
    lib = gp._densegp_gpu

    def state():
        th = lib.get_theta()
        p = gp.predict(Xs)
        return np.concatenate([th.get_mean(), th.get_data()]), lib.theta_fit_status(), lib.get_logpost(hat), p.mean, p.unc, p.deriv
    before = state()
    got = lib.predict_mixture(thetas, Xs, weights=np.ones(5), max_slots=2)
    assert got[5].all()
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)
    assert np.array_equal(before[0], hat)


def test_a_fit_after_the_call_is_the_fit_without_it():
    """the replica engine the call leaves in the cache is taken by the next multi-start fit: same seed, same optimum, bit for bit"""
    X, t, Xs = _data(30, 2, 5)
    thetas = _thetas(4, "Matern52", 2, False, False)
    out = []
    try:
        for call_first in (True, False):
            LibGPGPU.set_fit_options(max_iter=200, ftol=1e-9, gtol=1e-6, seed=5)
            gp = _gp(X, t, "Matern52", 1e-4)
            gp.fit(thetas[0])
            if call_first:
                gp._densegp_gpu.predict_mixture(thetas, Xs, weights=np.ones(4))
            M.fit_GP_MAP(gp, n_tries=4)
            th = gp.theta
            out.append((np.concatenate([th.get_mean(), th.get_data()]), gp.current_logpost, gp.predict(Xs).mean))
    finally:
        LibGPGPU.set_fit_options(max_iter=200, ftol=1e-9, gtol=1e-6, seed=0)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_a_sample_that_cannot_be_factorised_gets_weight_zero():
    """a fixed nugget of 0 with a length scale far beyond the design: every entry of the matrix is sigma^2 to rounding (the refused input of
    test_gpu_hessian).  That sample gets ok = 0 and weight 0, the others renormalise; all samples failing gives NaN, not an exception."""
    X, t, Xs = _data(130, 4, 37)
    good = np.array([3., 3.5, 3., 3.5, 0.2])
    bad = np.array([-60., -60., -60., -60., 0.])
    gp = _gp(X, t, "SquaredExponential", 0.)
    gp.fit(good)
    lib = gp._densegp_gpu
    thetas = np.array([bad, good, bad, good + 0.1, good - 0.1])
    w = np.array([5., 1., 1., 2., 0.5])
    got = lib.predict_mixture(thetas, Xs, weights=w)
    assert list(got[5]) == [False, True, False, True, True]
    assert got[3][0] == 0. and got[3][2] == 0. and np.isnan(got[4][0]) and np.isnan(got[4][2])
    # the restatement over the surviving samples (its own Cholesky of the bad matrix may or may not break down: it is told)
    ref, bars = _reference(X, t, thetas, Xs, "SquaredExponential", "zero", False, [None, 0., None, 0., 0.], w, None, True, "failed samples")
    assert list(ref["ok"]) == [False, True, False, True, True]
    _close(got, ref, bars, "failed samples")
    for a, b in zip(got, lib.predict_mixture(thetas, Xs, weights=w, max_slots=2, max_points=16)):
        assert np.array_equal(a, b, equal_nan=True)
    mean, within, between, wout, F, ok = lib.predict_mixture(np.array([bad, bad - 1.]), Xs, weights=np.ones(2))
    assert not ok.any() and all(np.all(np.isnan(a)) for a in (mean, within, between, wout, F))
    res = M.predict_marginal(gp, Xs, thetas=np.array([bad, bad - 1.]))
    assert np.isnan(res.ess) and np.all(np.isnan(res.unc))
    assert np.array_equal(gp.predict(Xs).mean, gp.predict(Xs).mean) and lib.theta_fit_status()


def test_an_adaptive_nugget_runs_its_ladder_per_sample():
    """five design points are repeated: no sample factorises without jitter, and an adaptive nugget finds each sample's own,
    sigma_s^2 x 1e-6 x 10^k.  The nugget a sample used is what include_nugget adds to its variance."""
    X, t, Xs = _data(30, 2, 37, repeats=5)
    S = 5
    thetas = _thetas(S, "Matern52", 2, False, False)
    gp = _gp(X, t, "Matern52", "adaptive")
    gp.fit(thetas[0])
    lib = gp._densegp_gpu
    fitted_nugget = gp.nugget
    assert fitted_nugget > 0.
    nugs = []
    for s in range(S):
        a = lib.predict_mixture(thetas[s:s + 1], Xs, weights=np.ones(1), include_nugget=True)
        b = lib.predict_mixture(thetas[s:s + 1], Xs, weights=np.ones(1), include_nugget=False)
        assert a[5][0] and np.array_equal(a[0], b[0])
        j = int(np.argmax(b[1]))
        used = a[1][j] - b[1][j]
        rungs = np.exp(thetas[s, 2]) * 1e-6 * 10. ** np.arange(5)
        k = int(np.argmin(np.abs(rungs - used)))
        assert abs(used - rungs[k]) <= 1e-9 * b[1][j] + 1e-3 * rungs[k], (used, rungs)
        nugs.append(float(rungs[k]))
    print("nuggets of the samples:", nugs)
    assert len(set(nugs)) == S                                                 # every sample its own
    w = _weights("nonuniform", S)
    ref, bars = _reference(X, t, thetas, Xs, "Matern52", "zero", False, nugs, w, None, True, "adaptive ladder")
    _close(lib.predict_mixture(thetas, Xs, weights=w), ref, bars, "adaptive ladder")
    assert gp.nugget == fitted_nugget                                          # the emulator's own jitter is the one its fit found


# n = 30, D = 2, Matern52, nugget 1e-4, the targets of _data: the Hessian of the restatement at PD has eigenvalues 4.4 .. 55, at SADDLE
# -27, 2.9, 36.  (With the targets of _small_multi: emulator 0 at PD 3.6 .. 85, emulator 1 at SADDLE 3.7 .. 104, emulator 2 at
# PD + 0.1 -105, 3.1, 74 -- the one whose Laplace approximation does not exist.)
PD = np.array([1.5, .5, -.5])
SADDLE = np.array([0., 0., 0.])


def test_importance_weights():
    X, t, Xs = _data(30, 2, 37)
    for th, sign in ((PD, 1), (SADDLE, -1)):
        assert sign * np.linalg.eigvalsh(hr.hessian(X, t, th, "Matern52", False, 1e-4))[0] > 1.
    gp = _gp(X, t, "Matern52", 1e-4)
    gp.fit(PD)
    S = 8
    res = M.predict_marginal(gp, Xs, n_samples=S, rng=7, importance=True)
    lap = M.laplace_approximation(gp)
    assert lap.is_minimum and res.laplace_ok is True
    assert np.array_equal(res.thetas, lap.sample(S, rng=7))
    q = lap.logpdf(res.thetas)
    ref, bars = _reference(X, t, res.thetas, Xs, "Matern52", "zero", False, 1e-4, None, q, True, "importance")
    assert res.ok.all()
    _close((res.mean, res.within, res.between, res.weights), ref, bars, "importance")
    w, ess = M.mixture_weights(ref["F"], ref["ok"], log_q=q)
    pos = w > 0
    assert np.array_equal(res.weights > 0, pos)
    assert float(np.abs(np.log(res.weights[pos]) - np.log(w[pos])).max()) <= bars["logw"]
    assert abs(res.ess - ess) <= 2. * bars["logw"] * ess
    assert 1. <= res.ess <= S
    # the same samples through the explicit call
    got = gp._densegp_gpu.predict_mixture(res.thetas, Xs, log_q=q)
    for a, b in zip((res.mean, res.within, res.between, res.weights, res.logpost, res.ok), got):
        assert np.array_equal(a, b)
    uni = M.predict_marginal(gp, Xs, n_samples=S, rng=7, importance=False)
    assert np.array_equal(uni.thetas, res.thetas) and np.array_equal(uni.weights, np.full(S, 1. / S)) and uni.ess == S
    gp.fit(SADDLE)
    with pytest.raises(ValueError, match="positive definite"):
        M.predict_marginal(gp, Xs, n_samples=S, rng=7)


def _small_multi(devices=None):
    X, _, Xs = _data(30, 2, 37)
    rng = np.random.default_rng(9)
    T = np.array([np.sin(3 * X[:, 0] + .3 * k) + X[:, 1] ** 2 + .1 * rng.standard_normal(30) for k in range(4)])
    mo = M.MultiOutputGP_GPU(X, T, kernel="Matern52", nugget=1e-4, priors=GPPriors(n_corr=2, nugget_type="fixed"), devices=devices)
    mo.fit_emulator(0, PD)
    mo.fit_emulator(1, SADDLE)
    mo.fit_emulator(2, PD + 0.1)
    S = 5
    thetas = np.array([PD + 0.2 * np.random.default_rng(40 + e).standard_normal((S, 3)) for e in range(4)])
    w = np.array([_weights("nonuniform", S) + e for e in range(4)])
    return X, T, Xs, mo, thetas, w


def test_multi_output():
    X, T, Xs, mo, thetas, w = _small_multi()
    lib = mo._mogp_gpu
    assert mo.get_indices_fit() == [0, 1, 2]
    got = lib.predict_mixture(thetas, Xs, weights=w)
    assert list(got[6]) == [True, True, True, False]
    for a in got[:5]:
        assert np.all(np.isnan(a[3]))                                          # emulator 3 is not fit
    assert not got[5][3].any()
    for e in range(3):
        single = lib.emulator(e).predict_mixture(thetas[e], Xs, weights=w[e])
        for a, b in zip(got[:6], single):
            assert np.array_equal(a[e], b)
    ref, bars = _reference(X, T[1], thetas[1], Xs, "Matern52", "zero", False, 1e-4, w[1], None, True, "emulator 1 of 4")
    _close([a[1] for a in got[:4]], ref, bars, "emulator 1 of 4")
    assert mo.get_indices_fit() == [0, 1, 2]
    # Laplace draws: emulator 2 sits at a point where its Hessian is not positive definite and is predicted at its fitted theta alone;
    # emulator 3 is not fit
    S = 5
    hats = [PD, SADDLE, PD + 0.1]
    ev = [np.linalg.eigvalsh(hr.hessian(X, T[e], hats[e], "Matern52", False, 1e-4))[0] for e in range(3)]
    assert ev[0] > 1. and ev[1] > 1. and ev[2] < -1.
    for importance in (True, False):
        res = M.predict_marginal(mo, Xs, n_samples=S, rng=3, importance=importance)
        assert list(res.laplace_ok) == [True, True, False, False]
        plug = mo.predict(Xs, deriv=False, allow_not_fit=True)
        assert_array_equal(res.mean[2], plug.mean[2])
        assert_array_equal(res.unc[2], plug.unc[2])
        assert not res.between[2].any() and list(res.weights[2]) == [1., 0., 0., 0., 0.] and res.ess[2] == 1.
        assert np.array_equal(res.thetas[2], np.tile(PD + 0.1, (S, 1)))
        assert np.all(np.isnan(res.mean[3])) and np.all(np.isnan(res.weights[3])) and np.isnan(res.ess[3])
        assert res.mean.shape == (4, 37) and res.weights.shape == (4, S) and res.ess.shape == (4,)
        laps = M.laplace_approximation(mo)
        rng = np.random.default_rng(3)
        assert np.array_equal(res.thetas[0], laps[0].sample(S, rng)) and np.array_equal(res.thetas[1], laps[1].sample(S, rng))
        assert res.between[0].max() > 0 and 1. <= res.ess[0] <= S
        if not importance:
            assert np.array_equal(res.weights[0], np.full(S, 1. / S))


def test_two_parts_on_one_device_are_the_one_part_model():
    X, T, Xs, mo, thetas, w = _small_multi()
    _, _, _, two, _, _ = _small_multi(devices=[0, 0])
    assert len(two.devices) == 2
    q = np.random.default_rng(2).standard_normal(w.shape)
    for kw in (dict(weights=w), dict(log_q=q), dict(weights=w, max_slots=3, max_points=16)):
        for a, b in zip(mo._mogp_gpu.predict_mixture(thetas, Xs, **kw), two._mogp_gpu.predict_mixture(thetas, Xs, **kw)):
            assert np.array_equal(a, b, equal_nan=True)


def test_refusals():
    X, t, Xs = _data(33, 3, 5)
    th = _thetas(3, "SquaredExponential", 3, False, False)
    gp = M.GaussianProcessGPU(X, t, nugget="pivot", priors=GPPriors(n_corr=3, nugget_type="pivot"))
    gp.fit(th[0])
    with pytest.raises(RuntimeError, match="pivot"):
        gp._densegp_gpu.predict_mixture(th, Xs, weights=np.ones(3))
    with pytest.raises(RuntimeError, match="pivot"):
        M.predict_marginal(gp, Xs, thetas=th)
    gp = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", nugget=1e-4, analytic_mean=True)
    gp.fit(th[0])
    with pytest.raises(RuntimeError, match="analytic_mean"):
        gp._densegp_gpu.predict_mixture(th, Xs, weights=np.ones(3))
    gp = _gp(X, t, "SquaredExponential", 1e-4)
    lib = gp._densegp_gpu
    with pytest.raises(RuntimeError, match="not been fit"):
        lib.predict_mixture(th, Xs, weights=np.ones(3))
    with pytest.raises(ValueError, match="not been fit"):
        M.predict_marginal(gp, Xs, thetas=th)
    gp.fit(th[0])
    ok = lib.predict_mixture(th, Xs, weights=np.ones(3))
    assert ok[5].all()
    for kw in (dict(), dict(weights=np.ones(3), log_q=np.zeros(3))):           # neither, both
        with pytest.raises(RuntimeError, match="exactly one"):
            lib.predict_mixture(th, Xs, **kw)
    for bad in (np.array([1., -1., 1.]), np.array([1., np.nan, 1.]), np.array([1., np.inf, 1.])):
        with pytest.raises(RuntimeError, match="weights"):
            lib.predict_mixture(th, Xs, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            M.predict_marginal(gp, Xs, thetas=th, weights=bad)
    with pytest.raises(RuntimeError, match="log_q"):
        lib.predict_mixture(th, Xs, log_q=np.array([0., np.nan, 0.]))
    with pytest.raises(RuntimeError, match="shape"):
        lib.predict_mixture(th, Xs, weights=np.ones(4))
    with pytest.raises(RuntimeError, match="Shape"):
        lib.predict_mixture(np.zeros((3, 5)), Xs, weights=np.ones(3))          # one column too many
    with pytest.raises(RuntimeError, match="D columns"):
        lib.predict_mixture(th, np.zeros((5, 4)), weights=np.ones(3))
    with pytest.raises(RuntimeError, match="at least one sample"):
        lib.predict_mixture(np.zeros((0, 4)), Xs, weights=np.ones(0))
    bad_th = th.copy()
    bad_th[1, 0] = np.inf
    with pytest.raises(RuntimeError, match="finite"):
        lib.predict_mixture(bad_th, Xs, weights=np.ones(3))
    with pytest.raises(ValueError):
        M.predict_marginal(gp, np.zeros((5, 4)), thetas=th)
    for a, b in zip(ok, lib.predict_mixture(th, Xs, weights=np.ones(3))):      # nothing of the refused calls is left behind
        assert np.array_equal(a, b)
