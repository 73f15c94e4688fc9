"""Cross-validation at the fitted hyperparameters on the MI355X (mogp_emulator_amd.cross_validate, DenseGP_GPU / MultiOutputGP_GPU
.cross_validate, csrc/kernels_cv.hip) against the NumPy restatement (cv_restate.py), at the smallest shapes that cross the layout's edges:
n = 7 (one partial tile), 33, 130 with k = 5 (folds of 26), 257 with k = 2 (folds of 129 and 128: a sub-matrix of 256 rows, one padded
fold) and the stored n = 200 case with k = 10.

Tolerance.  Not fixed in advance: for every case the restatement is evaluated in float64 and in np.longdouble on the CPU, and the device is
allowed 100 x their disagreement, relative to the largest entry of each quantity (mean, variance, Mahalanobis distance, log score).  A
disagreement below the spacing of float64 counts as one spacing, 2^-52.  A case whose disagreement exceeds 1e-8 would be too
ill-conditioned to judge a kernel with; every case asserts that it is not.  Measured disagreements (this file prints them): DESIGN.md
section 4.
"""
import ctypes
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, _capi
from mogp_emulator_amd.Priors import GPPriors
from conftest import load_golden

import cv_restate as cr
from marginal_restate import UNIFORM

pytestmark = pytest.mark.gpu
MARGIN = 100.
ILL = 1e-8
EPS = 2. ** -52
LD = np.longdouble


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _data(n, D, repeats=0):
    rng = np.random.default_rng(11 + 1000 * n + D)
    X = rng.random((n, D))
    if repeats:
        X[n - repeats:] = X[:repeats]
    t = np.sin(3 * X[:, 0]) + (X[:, 1] ** 2 if D > 1 else 0.)
    if not repeats:
        t = t + .1 * rng.standard_normal(n)
    return X, t


def _nc(kernel, D):
    return 1 if kernel in UNIFORM else D


def _theta(kernel, D, fit, const):
    """correlation lengths of 0.1 - 0.6 times sqrt(D) (test_gpu_hessian._theta): the matrices stay well conditioned"""
    nc = _nc(kernel, D)
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, nc) if nc > 1 else np.array([np.log(1. / D) + 2.5])
    return np.concatenate([[0.2] if const else [], corr, [0.2], [-4.] if fit else []])


def _mean_arg(mean):
    if mean == "const":
        return LibGPGPU.ConstMeanFunc()
    if mean == "zero":
        return None
    return LibGPGPU.FixedMeanFunc(mean[1])


def _nugget_kind(nugget):
    return "fixed" if isinstance(nugget, float) else nugget


def _gp(X, t, kernel, nugget, mean="zero", **kw):
    return M.GaussianProcessGPU(X, t, mean=_mean_arg(mean), kernel=kernel, nugget=nugget,
                                priors=GPPriors(n_corr=_nc(kernel, X.shape[1]), nugget_type=_nugget_kind(nugget)), **kw)


def _labels(n, k, shuffled):
    if k is None:
        return np.arange(n), n
    return (M.kfold_labels(n, k, rng=5) if shuffled else M.kfold_labels(n, k)), k


def _bars(a, b, what):
    """float64 restatement a against long double b: the device's bars in absolute terms"""
    bars = {}
    for q, (dis, scale) in cr.disagreement(a, b).items():
        assert dis <= ILL, "the case is too ill-conditioned to test a kernel with (%s: %.3g)" % (q, dis)
        bars[q] = MARGIN * max(dis, EPS) * scale
        print("%s: float64 vs long double, %s %.3g of %.4g" % (what, q, dis, scale))
    return bars


@functools.lru_cache(maxsize=None)
def _reference(form, n, D, k, shuffled, kernel, nugget, mean, eta=None):
    """(float64 restatement, bars) of a case; nugget "adaptive": eta is the jitter the fit found"""
    X, t = _data(n, D, repeats=5 if eta else 0)
    fit = nugget == "fit"
    theta = _theta(kernel, D, fit, mean == "const")
    labels, kk = _labels(n, k, shuffled)
    nug = None if fit else ((eta or 0.) if nugget == "adaptive" else nugget)
    f = cr.fast if form == "fast" else cr.brute
    a = f(X, t, theta, labels, kk, kernel, mean, fit, nug)
    b = f(X, t, theta, labels, kk, kernel, mean, fit, nug, dtype=LD)
    what = "%s n=%d D=%d %s %s %s %s" % (form, n, D, "loo" if k is None else "k=%d" % k, kernel, nugget, mean)
    return a, _bars(a, b, what)


def _close(res, ref, bars, what, include_nugget=True):
    eta = float(ref["eta"])
    want = {"mean": ref["mean"], "var": ref["var"] if include_nugget else np.maximum(ref["var"] - eta, 0.),
            "mahalanobis": ref["mahalanobis"], "log_score": ref["log_score"]}
    got = {"mean": res.mean, "var": res.unc, "mahalanobis": res.mahalanobis, "log_score": res.log_score}
    assert np.all(res.ok)
    for q in cr.QUANTITIES:
        assert got[q].shape == want[q].shape and np.all(np.isfinite(got[q]))
        err = float(np.abs(got[q] - want[q]).max())
        print("%s: device vs float64 restatement, %s %.3g (bar %.3g)" % (what, q, err, bars[q]))
        assert err <= bars[q], (what, q, err, bars[q])


# (n, D, k (None: leave-one-out), shuffled labels, kernel, nugget, mean)
PARITY = [
    (7, 1, None, False, "SquaredExponential", 1e-4, "zero"),
    (7, 3, 3, True, "Matern52", "fit", "const"),
    (33, 3, None, False, "UniformMat52", 1e-4, ("fixed", 0.3)),
    (33, 1, 3, False, "SquaredExponential", 1e-4, "zero"),
    (33, 3, 4, True, "UniformSqExp", "fit", "zero"),
    (130, 3, 5, True, "SquaredExponential", 1e-4, "zero"),
    (130, 3, 5, False, "Matern52", "fit", "const"),
    (130, 3, None, False, "Matern52", "adaptive", "zero"),
    (257, 4, 2, False, "Matern52", 1e-4, "zero"),
]


def _case_id(c):
    return "n%d-D%d-%s-%s-%s-%s-%s" % (c[0], c[1], "loo" if c[2] is None else "k%d" % c[2], "shuffled" if c[3] else "mod", c[4], c[5],
                                       c[6] if isinstance(c[6], str) else "fixedmean")


def _fitted(case):
    n, D, k, shuffled, kernel, nugget, mean = case
    X, t = _data(n, D)
    gp = _gp(X, t, kernel, nugget, mean)
    gp.fit(_theta(kernel, D, nugget == "fit", mean == "const"))
    return gp


@pytest.mark.parametrize("case", PARITY, ids=_case_id)
def test_device_matches_restatement(case):
    n, D, k, shuffled, kernel, nugget, mean = case
    ref, bars = _reference("fast", *case)
    gp = _fitted(case)
    if nugget == "adaptive":
        assert gp.nugget == 0.                       # a well-conditioned matrix factorises without jitter
    labels, kk = _labels(n, k, shuffled)
    for include_nugget in (True, False):
        if k is None:
            res = M.cross_validate(gp, include_nugget=include_nugget)
        elif shuffled:
            res = M.cross_validate(gp, k=k, rng=5, include_nugget=include_nugget)
        else:
            res = M.cross_validate(gp, k=k, include_nugget=include_nugget)
        assert np.array_equal(res.folds, labels) and res.k == kk and res.mean.shape == (n,) and res.log_score.shape == (kk,)
        _close(res, ref, bars, _case_id(case), include_nugget)
        se = (res.mean - gp.targets) / np.sqrt(ref["var"])
        assert float(np.abs(res.standard_errors - se).max()) <= 1e-6 * float(np.abs(se).max())
        assert abs(res.rmse - np.sqrt(np.mean((ref["mean"] - gp.targets) ** 2))) <= bars["mean"]
        assert abs(res.total_log_score - ref["log_score"].sum()) <= kk * bars["log_score"]


@pytest.mark.parametrize("tag", ["Matern52_fit", "SquaredExponential_fit"])
def test_stored_case_n200_k10(tag):
    """the stored n = 200, D = 4 case at the reference's own fitted theta, k = 10: 10 sub-matrices of 20 points"""
    g = load_golden("c1_n200_d4.npz")
    kernel = tag.split("_")[0]
    X, t, theta = g["X"], g["T"][0], g[tag + "_theta"]
    labels = M.kfold_labels(200, 10)
    a = cr.fast(X, t, theta, labels, 10, kernel, "zero", True, None)
    b = cr.fast(X, t, theta, labels, 10, kernel, "zero", True, None, dtype=LD)
    bars = _bars(a, b, "c1_n200_d4 " + tag)
    gp = _gp(X, t, kernel, "fit")
    gp.fit(theta)
    _close(M.cross_validate(gp, k=10), a, bars, "c1_n200_d4 " + tag)
    _close(M.cross_validate(gp, k=10, include_nugget=False), a, bars, "c1_n200_d4 " + tag, False)


def test_repeated_design_points_under_the_adaptive_ladder():
    """five design points are repeated: the matrix factorises only with jitter, and eta is the jitter the fit found"""
    n, D, k, kernel = 30, 2, 3, "Matern52"
    X, t = _data(n, D, repeats=5)
    gp = _gp(X, t, kernel, "adaptive")
    theta = _theta(kernel, D, False, False)
    gp.fit(theta)
    eta = float(gp.nugget)
    rungs = np.exp(theta[D]) * 1e-6 * 10. ** np.arange(5)
    assert eta > 0. and np.min(np.abs(rungs - eta)) <= 1e-12 * eta
    for kk in (k, None):
        ref, bars = _reference("fast", n, D, kk, False, kernel, "adaptive", "zero", eta)
        _close(M.cross_validate(gp, k=kk), ref, bars, "adaptive ladder")
        _close(M.cross_validate(gp, k=kk, include_nugget=False), ref, bars, "adaptive ladder", False)
    assert gp.nugget == eta


def test_against_refits_on_the_device():
    """end to end: a GaussianProcessGPU on the other four folds at the same theta predicts the held-out fold.  The refit's own rounding
    is that of the brute-force restatement, so the bar is 100 x ITS float64-against-long-double disagreement."""
    case = (130, 3, 5, True, "SquaredExponential", 1e-4, "zero")
    n, D, k, shuffled, kernel, nugget, mean = case
    ref, bars = _reference("brute", *case)
    X, t = _data(n, D)
    theta = _theta(kernel, D, False, False)
    gp = _fitted(case)
    res = M.cross_validate(gp, k=k, rng=5)
    _close(res, ref, bars, "device vs brute-force restatement")
    labels, _ = _labels(n, k, shuffled)
    for f in range(k):
        F = labels == f
        part = _gp(X[~F], t[~F], kernel, nugget)
        part.fit(theta)
        p = part.predict(X[F], deriv=False, include_nugget=True)
        for q, got, want in (("mean", res.mean[F], p.mean), ("var", res.unc[F], p.unc)):
            err = float(np.abs(got - want).max())
            print("fold %d: cross_validate vs refit + predict on the device, %s %.3g (bar %.3g)" % (f, q, err, bars[q]))
            assert err <= bars[q], (f, q, err, bars[q])


@pytest.mark.parametrize("case", [(33, 3, None, False, "UniformMat52", 1e-4, ("fixed", 0.3)), (130, 3, None, False, "Matern52", "adaptive", "zero")],
                         ids=_case_id)
def test_single_point_folds_through_the_kfold_path(case):
    """max fold size 1 takes the leave-one-out kernel whatever the labels; folds of one and two points take the sub-engine.  Both agree
    with the restatement, and on the points that are alone in their fold with each other."""
    n = case[0]
    ref, bars = _reference("fast", *case)
    gp = _fitted(case)
    loo = M.cross_validate(gp)
    same = M.cross_validate(gp, folds=np.arange(n))
    for q in ("mean", "unc", "mahalanobis", "log_score"):
        assert float(np.abs(getattr(same, q) - getattr(loo, q)).max()) <= bars["var" if q == "unc" else q]
    perm = np.random.default_rng(2).permutation(n)
    via = M.cross_validate(gp, folds=perm)                   # a permutation: still leave-one-out, the scalars land at the labels
    assert np.array_equal(via.mean, loo.mean) and np.array_equal(via.unc, loo.unc)
    assert np.array_equal(via.log_score[perm], loo.log_score) and np.array_equal(via.mahalanobis[perm], loo.mahalanobis)
    # the k-fold path on single points: the last two points share a fold, every other fold is one point
    folds = np.minimum(np.arange(n), n - 2)
    sub = gp._densegp_gpu.cross_validate(folds, n - 1)
    one = np.arange(n - 2)
    for q, got, want in (("mean", sub[0][one], loo.mean[one]), ("var", sub[1][one], loo.unc[one]),
                         ("mahalanobis", sub[2][one], loo.mahalanobis[one]), ("log_score", sub[3][one], loo.log_score[one])):
        err = float(np.abs(got - want).max())
        print("single-point folds through the sub-engine vs the leave-one-out kernel, %s %.3g (bar %.3g)" % (q, err, bars[q]))
        assert err <= bars[q], (q, err, bars[q])
    assert sub[4].all()


def _multi(E, n=130, D=3, kernel="Matern52", nugget=1e-4, devices=None, fit=None):
    X, _ = _data(n, D)
    rng = np.random.default_rng(9)
    T = np.array([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 + .1 * rng.standard_normal(n) for k in range(E)])
    mo = M.MultiOutputGP_GPU(X, T, kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_nugget_kind(nugget)), devices=devices)
    theta = _theta(kernel, D, False, False)
    for e in (range(E) if fit is None else fit):
        mo.fit_emulator(e, theta + 0.05 * e)
    return X, T, mo, theta


def test_determinism_and_grouping():
    n, k = 130, 5
    X, T, mo, theta = _multi(3)
    first = M.cross_validate(mo, k=k, rng=5)
    again = M.cross_validate(mo, k=k, rng=5)
    names = ("mean", "unc", "mahalanobis", "log_score", "ok")
    for q in names:
        assert np.array_equal(getattr(first, q), getattr(again, q)), q                 # two identical calls: the same bits
    labels = M.kfold_labels(n, k, rng=5)
    a = cr.fast(X, T[1], theta + 0.05, labels, k, "Matern52", "zero", False, 1e-4)
    b = cr.fast(X, T[1], theta + 0.05, labels, k, "Matern52", "zero", False, 1e-4, dtype=LD)
    bars = _bars(a, b, "emulator 1 of 3")
    for max_slots in (1, 3):
        got = M.cross_validate(mo, k=k, rng=5, max_slots=max_slots)
        equal = all(np.array_equal(getattr(first, q), getattr(got, q)) for q in names)
        print("max_slots=%d: bit-equal to the default grouping: %s" % (max_slots, equal))
        for q, name in (("mean", "mean"), ("var", "unc"), ("mahalanobis", "mahalanobis"), ("log_score", "log_score")):
            err = float(np.abs(getattr(got, name)[1] - getattr(first, name)[1]).max())
            assert err <= bars[q], (max_slots, q, err, bars[q])
        assert got.ok.all()


def _counter(name):
    c = ctypes.c_longlong(0)
    assert _capi.load().mogp_profile_counter(name.encode(), ctypes.byref(c)) == 0
    return c.value


def test_engine_state_survives_the_call():
    case = (130, 3, 5, True, "Matern52", "fit", "const")
    n, D, k, shuffled, kernel, nugget, mean = case
    X, t = _data(n, D)
    Xs = np.random.default_rng(1).random((37, D))
    theta = _theta(kernel, D, True, True)
    gp = _fitted(case)
    th0 = np.concatenate([gp.theta.get_mean(), gp.theta.get_data()])
    lp0, p0 = gp.current_logpost, gp.predict(Xs)
    M.cross_validate(gp, k=k)
    live1 = _counter("device_bytes_live")
    M.cross_validate(gp, k=k)
    assert _counter("device_bytes_live") == live1                                        # the sub-engine and the scratch are gone
    M.cross_validate(gp)
    assert np.array_equal(np.concatenate([gp.theta.get_mean(), gp.theta.get_data()]), th0) and gp.current_logpost == lp0
    p1 = gp.predict(Xs)
    assert np.array_equal(p1.mean, p0.mean) and np.array_equal(p1.unc, p0.unc) and np.array_equal(p1.deriv, p0.deriv)
    # a fit after the call is the fit without it
    gp.fit(theta + 0.1)
    fresh = _gp(X, t, kernel, nugget, mean)
    fresh.fit(theta + 0.1)
    assert gp.current_logpost == fresh.current_logpost
    pa, pb = gp.predict(Xs), fresh.predict(Xs)
    assert np.array_equal(pa.mean, pb.mean) and np.array_equal(pa.unc, pb.unc)
    ra, rb = M.cross_validate(gp, k=k), M.cross_validate(fresh, k=k)
    assert np.array_equal(ra.mean, rb.mean) and np.array_equal(ra.log_score, rb.log_score)


def test_multi_output():
    n, k = 130, 5
    X, T, mo, theta = _multi(4, fit=(0, 1, 2))
    assert mo.get_indices_fit() == [0, 1, 2]
    a = cr.fast(X, T[1], theta + 0.05, M.kfold_labels(n, k), k, "Matern52", "zero", False, 1e-4)
    b = cr.fast(X, T[1], theta + 0.05, M.kfold_labels(n, k), k, "Matern52", "zero", False, 1e-4, dtype=LD)
    bars = _bars(a, b, "emulator 1 of 4")
    for kk in (k, None):
        res = M.cross_validate(mo, k=kk)
        K = n if kk is None else kk
        assert res.mean.shape == (4, n) and res.log_score.shape == (4, K) and res.ok.shape == (4, K)
        for arr in (res.mean, res.unc, res.mahalanobis, res.log_score, res.standard_errors):
            assert np.all(np.isnan(arr[3])) and np.all(np.isfinite(arr[:3]))              # emulator 3 is not fit
        assert not res.ok[3].any() and res.ok[:3].all() and np.isnan(res.rmse[3]) and np.isnan(res.total_log_score[3])
        for e in range(3):
            single = M.cross_validate(mo.emulators[e], k=kk)
            for q, name in (("mean", "mean"), ("var", "unc"), ("mahalanobis", "mahalanobis"), ("log_score", "log_score")):
                err = float(np.abs(getattr(res, name)[e] - getattr(single, name)).max())
                assert err <= bars[q], (e, q, err, bars[q])
            assert single.ok.all()
        if kk is not None:
            _close(M.CrossValidationResult(res.folds, T[1], res.mean[1], res.unc[1], res.mahalanobis[1], res.log_score[1], res.ok[1],
                                           1e-4, True), a, bars, "emulator 1 of 4")
    assert mo.get_indices_fit() == [0, 1, 2]
    # the others are unchanged by the one that is not fit
    _, _, full, _ = _multi(3)
    r3, r4 = M.cross_validate(full, k=k), M.cross_validate(mo, k=k)
    for name in ("mean", "unc", "mahalanobis", "log_score"):
        err = float(np.abs(getattr(r3, name) - getattr(r4, name)[:3]).max())
        assert err <= bars["mean" if name == "mean" else ("var" if name == "unc" else name)] , (name, err)


def test_more_than_512_small_sub_matrices():
    """180 emulators x 3 folds of 11 points: 540 sub-matrices of one 128-tile, past the 512 up to which a batch of single-tile matrices
    takes the one-launch factorisation -- the sub-engine runs a multi-launch schedule"""
    n, D, k, E = 33, 3, 3, 180
    X, T, mo, theta = _multi(E, n=n, D=D, fit=())
    mo.fit(np.tile(theta, (E, 1)))
    res = M.cross_validate(mo, k=k)
    assert res.ok.all()
    for e in (0, 97, E - 1):
        a = cr.fast(X, T[e], theta, M.kfold_labels(n, k), k, "Matern52", "zero", False, 1e-4)
        b = cr.fast(X, T[e], theta, M.kfold_labels(n, k), k, "Matern52", "zero", False, 1e-4, dtype=LD)
        bars = _bars(a, b, "emulator %d of %d" % (e, E))
        _close(M.CrossValidationResult(res.folds, T[e], res.mean[e], res.unc[e], res.mahalanobis[e], res.log_score[e], res.ok[e], 1e-4, True),
               a, bars, "emulator %d of %d" % (e, E))


def test_two_parts_on_one_device_are_the_one_part_model():
    X, T, mo, theta = _multi(4, fit=(0, 1, 2))
    _, _, two, _ = _multi(4, fit=(0, 1, 2), devices=[0, 0])
    assert len(two.devices) == 2
    a = cr.fast(X, T[0], theta, M.kfold_labels(130, 5), 5, "Matern52", "zero", False, 1e-4)
    b = cr.fast(X, T[0], theta, M.kfold_labels(130, 5), 5, "Matern52", "zero", False, 1e-4, dtype=LD)
    bars = _bars(a, b, "emulator 0 of 4")
    for kw in (dict(k=5), dict(), dict(k=5, max_slots=3)):
        ra, rb = M.cross_validate(mo, **kw), M.cross_validate(two, **kw)
        assert np.array_equal(ra.ok, rb.ok)
        for q, name in (("mean", "mean"), ("var", "unc"), ("mahalanobis", "mahalanobis"), ("log_score", "log_score")):
            x, y = getattr(ra, name), getattr(rb, name)
            assert np.array_equal(np.isnan(x), np.isnan(y))
            assert float(np.nanmax(np.abs(x - y))) <= bars[q], (kw, q)


def test_refusals():
    X, t = _data(33, 3)
    th = _theta("SquaredExponential", 3, False, False)
    gp = M.GaussianProcessGPU(X, t, nugget="pivot", priors=GPPriors(n_corr=3, nugget_type="pivot"))
    gp.fit(th)
    with pytest.raises(RuntimeError, match="pivot"):
        M.cross_validate(gp, k=3)
    with pytest.raises(RuntimeError, match="pivot"):
        gp._densegp_gpu.cross_validate(np.arange(33) % 3, 3)
    gp = M.GaussianProcessGPU(X, t, mean="c+c*x[0]", nugget=1e-4, analytic_mean=True)
    gp.fit(th)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        M.cross_validate(gp, k=3)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        gp._densegp_gpu.cross_validate(np.arange(33) % 3, 3)
    gp = _gp(X, t, "SquaredExponential", 1e-4)
    with pytest.raises(RuntimeError, match="not been fit"):
        M.cross_validate(gp, k=3)
    with pytest.raises(RuntimeError, match="not been fit"):
        gp._densegp_gpu.cross_validate(np.arange(33) % 3, 3)
    gp.fit(th)
    ok = M.cross_validate(gp, k=3)
    lib = gp._densegp_gpu
    for k in (1, 0, 34, -2):
        with pytest.raises(ValueError):
            M.cross_validate(gp, k=k)
        with pytest.raises(RuntimeError, match="number of folds"):
            lib.cross_validate(np.zeros(33, dtype=int), k)
    for labels, k in ((np.arange(33) % 3 - 1, 3), (np.arange(33) % 4, 3)):
        with pytest.raises(ValueError):
            M.cross_validate(gp, folds=labels, k=k)
        with pytest.raises(RuntimeError, match="outside"):
            lib.cross_validate(labels, k)
    with pytest.raises(ValueError):
        M.cross_validate(gp, folds=np.array([0, 2] * 16 + [0]))
    with pytest.raises(RuntimeError, match="empty"):
        lib.cross_validate(np.array([0, 2] * 16 + [0]), 3)
    with pytest.raises(RuntimeError, match="one fold label per training point"):
        lib.cross_validate(np.arange(32) % 3, 3)
    with pytest.raises(RuntimeError, match="max_slots"):
        lib.cross_validate(np.arange(33) % 3, 3, max_slots=-1)
    again = M.cross_validate(gp, k=3)                                                  # nothing of the refused calls is left behind
    assert np.array_equal(ok.mean, again.mean) and np.array_equal(ok.log_score, again.log_score)
