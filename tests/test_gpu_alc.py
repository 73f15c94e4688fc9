"""The posterior cross covariance and the ALC criterion on the MI355X (mogp_emulator_amd.ActiveLearning, csrc/kernels_alc.hip) at shapes
that sit on the tile edges: n = 130, D = 3, E = 3 emulators with a different theta each, squared exponential and Matern-5/2, a fixed
nugget 1e-2 and a fitted nugget e^-4, m_c in {1, 127, 128, 129, 300} candidates against m_r in {1, 128, 129, 300} reference points; one
case each with D = 80 (the epilogue's slices of dimensions), UniformSqExp and ProductMat52.

Every bar is derived, not measured (alc_restate.py has the formulas): per entry of the covariance
    4 n 2^-52 cond_2(Q) |k(x_i)|_2 |Q^-1 k(x'_j)|_2 + (D + 4) 2^-52 sigma^2,
propagated to ALC to first order; (m_r + 4) 2^-52 relative for a sum of m_r non-negative terms against the same sum in another order.
The measured figures are printed as fractions of their bars.  Measured on an MI355X: see DESIGN.md section 3 "Active learning".
"""
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import alc_restate as ar

pytestmark = pytest.mark.gpu
EPS = 2. ** -52
N, D, E = 130, 3, 3
MCS = (1, 127, 128, 129, 300)
MRS = (1, 128, 129, 300)
KERNELS = ("SquaredExponential", "Matern52")
NUGGETS = ("fit", 1e-2)
MODELS = [(k, g) for k in KERNELS for g in NUGGETS]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _model_id(mk):
    return "%s-%s" % (mk[0], "fit" if mk[1] == "fit" else "fixed")


@functools.lru_cache(maxsize=None)
def _data(n=N, d=D):
    rng = np.random.default_rng(77 + d)
    X = rng.random((n, d))
    T = np.array([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 + .1 * rng.standard_normal(n) for k in range(E + 1)])
    return X, T


def _theta(e, fit, d=D, nc=None):
    """correlation lengths of 0.1 - 0.6 times sqrt(D), sigma^2 = e^0.2; a fitted nugget of e^-4"""
    nc = d if nc is None else nc
    corr = np.log(1. / d) + np.linspace(1.0, 3.2, nc) + 0.05 * e
    return np.concatenate([corr, [0.2 + 0.03 * e], [-4. + 0.1 * e] if fit else []])


def _kind(nugget):
    return "fixed" if isinstance(nugget, float) else nugget


def _eta(nugget, e):
    return float(np.exp(-4. + 0.1 * e)) if nugget == "fit" else float(nugget)


@functools.lru_cache(maxsize=None)
def _model(kernel, nugget, fit=None, devices=None):
    X, T = _data()
    mo = M.MultiOutputGP_GPU(X, T[:E], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)),
                             devices=None if devices is None else list(devices))
    for e in (range(E) if fit is None else fit):
        mo.fit_emulator(e, _theta(e, nugget == "fit"))
    return mo


@functools.lru_cache(maxsize=None)
def _single(kernel, nugget, e):
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[e], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)))
    gp.fit(_theta(e, nugget == "fit"))
    return gp


@functools.lru_cache(maxsize=None)
def _points(m, salt=0, d=D):
    x = np.random.default_rng(500 + m + 1000 * salt).random((m, d))
    x.setflags(write=False)
    return x


def _cand(m):
    return _points(m, 0)


def _ref(m):
    return _points(m, 1)


@functools.lru_cache(maxsize=None)
def _post(kernel, nugget, e):
    """the restatement's posterior of emulator e; computed once, never modified"""
    return ar.Posterior(_data()[0], _theta(e, nugget == "fit"), kernel, _eta(nugget, e))


@functools.lru_cache(maxsize=None)
def _restated(kernel, nugget, e, mc, mr):
    """(c (m_c, m_r), its bar) of the restatement"""
    p = _post(kernel, nugget, e)
    return p.cov(_cand(mc), _ref(mr)), p.cov_bar(_cand(mc), _ref(mr))


# ---- 1. predict_cov ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_predict_cov_against_the_restatement(mk):
    mo = _model(*mk)
    worst = 0.
    for mc in MCS:
        for mr in MRS:
            C = M.predict_cov(mo, _cand(mc), _ref(mr))
            assert C.shape == (E, mc, mr) and np.all(np.isfinite(C))
            for e in range(E):
                want, bar = _restated(*mk, e, mc, mr)
                frac = np.max(np.abs(C[e] - want) / bar)
                worst = max(worst, frac)
                assert frac <= 1., (mk, mc, mr, e, frac)
    print("%s: predict_cov off the restatement by at most %.3g of the entry bar" % (_model_id(mk), worst))


@pytest.mark.parametrize("m", MCS)
@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_predict_cov_of_a_set_with_itself(mk, m):
    mo = _model(*mk)
    X = _cand(m)
    C = M.predict_cov(mo, X)
    assert C.shape == (E, m, m) and np.array_equal(C, M.predict_cov(mo, X, X))
    full = mo.predict(X, full_cov=True, include_nugget=False, deriv=False).unc
    unc = mo.predict(X, include_nugget=False, deriv=False).unc
    for e in range(E):
        bar = _post(*mk, e).cov_bar(X, X)
        f1 = np.max(np.abs(C[e] - full[e]) / (2. * bar))
        f2 = np.max(np.abs(np.maximum(np.diag(C[e]), 0.) - unc[e]) / np.diag(bar))
        print("%s m=%d e=%d: against full_cov %.3g of twice the bar, diagonal against predict %.3g of the bar" % (_model_id(mk), m, e, f1, f2))
        assert f1 <= 1. and f2 <= 1.


@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_predict_cov_transposes(mk):
    mo = _model(*mk)
    for mc, mr in ((129, 300), (1, 128), (300, 1)):
        A, B = M.predict_cov(mo, _cand(mc), _ref(mr)), M.predict_cov(mo, _ref(mr), _cand(mc))
        for e in range(E):
            bar = _restated(*mk, e, mc, mr)[1]
            frac = np.max(np.abs(A[e] - B[e].T) / bar)
            print("%s %d x %d e=%d: c(X1, X2) against c(X2, X1)^T %.3g of the bar" % (_model_id(mk), mc, mr, e, frac))
            assert frac <= 1.


# ---- 2. alc_criterion ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _weights(mr):
    w = np.random.default_rng(9 + mr).random(mr) + .1
    w /= w.sum()
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_alc_against_the_devices_own_covariance_and_the_restatement(mk):
    mo = _model(*mk)
    worst_epi = worst = 0.
    for mc in MCS:
        for mr in MRS:
            cand, ref = _cand(mc), _ref(mr)
            for w in (None, _weights(mr)):
                r = M.alc_criterion(mo, cand, ref, weights=w)
                ww = np.full(mr, 1. / mr) if w is None else w
                assert r.reduction.shape == (E, mc) and r.cand_variance.shape == (E, mc) and r.ref_variance.shape == (E, mr)
                assert r.degenerate.shape == (E, mc) and r.degenerate.dtype == bool and r.noise.shape == (E,) and np.array_equal(r.weights, ww)
                assert np.array_equal(r.noise, mo._nuggets())
                # s^2 + tau >= tau >= 1e-2 >> the floor: nothing may be degenerate here
                assert r.degenerate.sum() == 0 and np.all(np.isfinite(r.reduction)) and np.all(r.reduction >= 0.)
                # the epilogue alone: the same sum from the device's own covariance and variances, in NumPy's order
                C = M.predict_cov(mo, cand, ref)
                own = (ww[None, None, :] * C ** 2).sum(axis=2) / (r.cand_variance + r.noise[:, None])
                frac = np.max(np.abs(r.reduction - own) / ((mr + 4) * EPS * own))
                worst_epi = max(worst_epi, frac)
                assert frac <= 1., (mk, mc, mr, frac)
                for e in range(E):
                    p = _post(*mk, e)
                    want, _, _, deg, Cr, d = ar.alc(p, cand, ref, ww, r.noise[e])
                    bar = ar.alc_bar(p, cand, ref, ww, Cr, d)
                    f = np.max(np.abs(r.reduction[e] - want) / bar)
                    worst = max(worst, f)
                    assert not deg.any() and f <= 1., (mk, mc, mr, e, f)
    print("%s: ALC off NumPy on the device's own covariance by at most %.3g of (m_r + 4) eps, off the restatement by at most %.3g of the "
          "propagated bar" % (_model_id(mk), worst_epi, worst))


def test_noise_argument():
    mk = MODELS[0]
    mo = _model(*mk)
    cand, ref = _cand(129), _ref(128)
    r0, r1 = M.alc_criterion(mo, cand, ref, noise=0.), M.alc_criterion(mo, cand, ref, noise=.25)
    assert np.array_equal(r0.noise, np.zeros(E)) and np.array_equal(r1.noise, np.full(E, .25))
    assert np.array_equal(r0.cand_variance, r1.cand_variance)
    np.testing.assert_allclose(r1.reduction * (r1.cand_variance + .25), r0.reduction * r0.cand_variance, rtol=8 * EPS)


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_one_hot_weights_and_a_single_point(mk):
    mo = _model(*mk)
    cand, ref = _cand(129), _ref(300)
    C = M.predict_cov(mo, cand, ref)
    for j in (0, 127, 128, 299):
        w = np.zeros(300)
        w[j] = 1.
        r = M.alc_criterion(mo, cand, ref, weights=w)
        want = C[:, :, j] ** 2 / (r.cand_variance + r.noise[:, None])
        assert np.all(np.abs(r.reduction - want) <= 5 * EPS * want), (mk, j)
    x = _cand(1)
    r = M.alc_criterion(mo, x, x)
    s2 = mo.predict(x, include_nugget=False, deriv=False).unc[:, 0]
    bar = np.array([_post(*mk, e).var_bar(x)[0] for e in range(E)])
    d = s2 + r.noise
    want = s2 ** 2 / d
    # c(x, x) against s^2(x): two evaluations of one number, each inside the entry bar
    tol = 2. * s2 * (2. * bar) / d + s2 ** 2 * bar / d ** 2
    print("%s: one point as both sets, |ALC - s^4 / (s^2 + tau)| / bar at most %.3g" % (_model_id(mk), np.max(np.abs(r.reduction[:, 0] - want) / tol)))
    assert np.all(np.abs(r.reduction[:, 0] - want) <= tol)
    assert np.array_equal(r.cand_variance[:, 0], s2) and np.array_equal(r.ref_variance[:, 0], s2)


# ---- 4. the conditioning identity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_conditioning_identity(mk):
    """A second model holds the training set plus candidate c*, at the same theta and nugget eta, and tau = eta: the weighted variance of
    its predictions over the reference points equals integrated_variance - reduction[c*]."""
    kernel, nugget = mk
    e = 1
    gp = _single(kernel, nugget, e)
    cand, ref, w = _cand(129), _ref(300), _weights(300)
    r = M.alc_criterion(gp, cand, ref, weights=w)            # noise = None: tau = the nugget of the fit = eta
    assert r.noise[0] == gp.nugget and abs(r.noise[0] - _eta(nugget, e)) <= 4 * EPS * _eta(nugget, e)
    p = _post(kernel, nugget, e)
    _, _, _, _, Cr, d = ar.alc(p, cand, ref, w, r.noise[0])
    abar = ar.alc_bar(p, cand, ref, w, Cr, d)
    X, T = _data()
    best = int(r.best[0])
    for c in sorted({best, 0, 128}):
        Xp = np.vstack([X, cand[c:c + 1]])
        g2 = M.GaussianProcessGPU(Xp, np.r_[T[e], 0.37], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)))
        g2.fit(_theta(e, nugget == "fit"))
        after = g2.predict(ref, include_nugget=False, deriv=False).unc @ w
        p2 = ar.Posterior(Xp, _theta(e, nugget == "fit"), kernel, _eta(nugget, e))
        bar = abar[c] + p2.var_bar(ref) @ w
        gap = abs(after - (r.integrated_variance[0] - r.reduction[0, c]))
        print("%s c*=%d%s: |sum w s2_new - (IV - ALC)| = %.3g, %.3g of the bar; ALC / IV = %.3g" %
              (_model_id(mk), c, " (argmax)" if c == best else "", gap, gap / bar, r.reduction[0, c] / r.integrated_variance[0]))
        assert gap <= bar


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return (np.array_equal(a.reduction, b.reduction, equal_nan=True) and np.array_equal(a.cand_variance, b.cand_variance, equal_nan=True) and
            np.array_equal(a.ref_variance, b.ref_variance, equal_nan=True) and np.array_equal(a.degenerate, b.degenerate))


@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_same_bits_whatever_the_cut(mk):
    mo = _model(*mk)
    for mc, mr in ((129, 300), (300, 129), (1, 1)):
        cand, ref, w = _cand(mc), _ref(mr), _weights(mr)
        base = M.alc_criterion(mo, cand, ref, weights=w)
        assert _same(base, M.alc_criterion(mo, cand, ref, weights=w))
        for mp in (128, 256, 0):
            for ms in (1, 0):
                assert _same(base, M.alc_criterion(mo, cand, ref, weights=w, max_points=mp, max_slots=ms)), (mk, mc, mr, mp, ms)
        C = M.predict_cov(mo, cand, ref)
        assert np.array_equal(C, M.predict_cov(mo, cand, ref)) and np.array_equal(C, M.predict_cov(mo, cand, ref, max_slots=1))
        for e in range(E):
            one = M.alc_criterion(_single(*mk, e), cand, ref, weights=w)
            assert one.reduction.shape == (1, mc)
            assert np.array_equal(one.reduction[0], base.reduction[e]) and np.array_equal(one.cand_variance[0], base.cand_variance[e])
            assert np.array_equal(one.ref_variance[0], base.ref_variance[e]) and one.noise[0] == base.noise[e]
            assert np.array_equal(M.predict_cov(_single(*mk, e), cand, ref)[0], C[e])


def test_same_bits_on_two_parts_of_one_device():
    mk = MODELS[1]
    mo, two = _model(*mk), _model(*mk, devices=(0, 0))
    cand, ref, w = _cand(300), _ref(129), _weights(129)
    assert _same(M.alc_criterion(mo, cand, ref, weights=w), M.alc_criterion(two, cand, ref, weights=w, max_points=128))
    assert np.array_equal(M.predict_cov(mo, cand, ref), M.predict_cov(two, cand, ref))


# ---- 6. a partly fitted model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_partly_fitted_model_and_the_variances_of_predict(mk):
    full, part = _model(*mk), _model(*mk, fit=(0, 2))
    cand, ref = _cand(300), _ref(129)
    a, b = M.alc_criterion(full, cand, ref), M.alc_criterion(part, cand, ref)
    for arr_a, arr_b in ((a.reduction, b.reduction), (a.cand_variance, b.cand_variance), (a.ref_variance, b.ref_variance)):
        assert np.all(np.isnan(arr_b[1])) and np.array_equal(arr_a[[0, 2]], arr_b[[0, 2]])
    assert not b.degenerate[1].any() and b.best[1] == 0
    assert np.array_equal(b.total(), (a.reduction[[0, 2]] / a.integrated_variance[[0, 2], None]).sum(axis=0))
    Ca, Cb = M.predict_cov(full, cand, ref), M.predict_cov(part, cand, ref)
    assert np.all(np.isnan(Cb[1])) and np.array_equal(Ca[[0, 2]], Cb[[0, 2]])
    # both variances are predict()'s own
    assert np.array_equal(a.cand_variance, full.predict(cand, include_nugget=False, deriv=False).unc)
    assert np.array_equal(a.ref_variance, full.predict(ref, include_nugget=False, deriv=False).unc)
    gp = _single(*mk, 2)
    one = M.alc_criterion(gp, cand, ref)
    assert np.array_equal(one.cand_variance[0], gp.predict(cand, include_nugget=False, deriv=False).unc)
    assert np.array_equal(one.ref_variance[0], gp.predict(ref, include_nugget=False, deriv=False).unc)


# ---- 7. the floor -------------------------------------------------------------------------------------------------------------------------

def test_candidates_on_training_points_without_nugget_are_degenerate():
    """Correlation lengths far below the spacing of the design: K is the identity to 1e-6 (cond_2 = 1), the adaptive nugget finds no
    jitter necessary, and s^2 at a training point is sigma^2 minus a sum of n squares that equals it to rounding -- at or below the floor
    (n + 2) 2^-52 sigma^2 by its derivation."""
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[0], nugget="adaptive")
    gp.fit(np.r_[np.full(D, 10.), 0.3])
    assert gp.nugget == 0.
    cand = np.vstack([X[:5], _cand(127), X[-3:]])
    on = np.r_[np.ones(5, bool), np.zeros(127, bool), np.ones(3, bool)]
    r = M.alc_criterion(gp, cand, _ref(129))
    assert r.noise[0] == 0.
    assert np.all(r.degenerate[0, on]) and np.all(r.reduction[0, on] == 0.) and not r.degenerate[0, ~on].any()
    assert np.all(np.isfinite(r.reduction)) and np.all(np.isfinite(r.cand_variance)) and np.all(np.isfinite(r.ref_variance))
    assert np.all(r.cand_variance[0, on] <= ar.floor_of(N, np.exp(0.3)))
    assert np.all(r.reduction[0, ~on] >= 0.)
    # with noise the same candidates are ordinary ones
    r2 = M.alc_criterion(gp, cand, _ref(129), noise=1e-3)
    assert not r2.degenerate.any() and np.all(np.isfinite(r2.reduction))


# ---- the other kernels, and an input wider than one slice of the epilogue ---------------------------------------------------------------------

@pytest.mark.parametrize("kernel,d", [("SquaredExponential", 80), ("UniformSqExp", 3), ("ProductMat52", 3), ("Matern52", 35)],
                         ids=["D80", "UniformSqExp", "ProductMat52", "D35"])
def test_other_kernels_and_dimension_slices(kernel, d):
    X, T = _data(N, d)
    nc = ar.n_corr(kernel, d)
    th = _theta(1, False, d, nc)
    if d > 3:       # correlation lengths relative to the diameter of the cube that keep k away from 0 and 1 in many dimensions
        th[:nc] = np.log(1. / d) + np.linspace(1.5, 3.5, nc)
    gp = M.GaussianProcessGPU(X, T[1], kernel=kernel, nugget=1e-2, priors=GPPriors(n_corr=nc, nugget_type="fixed"))
    gp.fit(th)
    p = ar.Posterior(X, th, kernel, 1e-2)
    cand, ref, w = _points(129, 0, d), _points(300, 1, d), _weights(300)
    C = M.predict_cov(gp, cand, ref)[0]
    want, bar = p.cov(cand, ref), p.cov_bar(cand, ref)
    f1 = np.max(np.abs(C - want) / bar)
    r = M.alc_criterion(gp, cand, ref, weights=w)
    own = (w[None, :] * C ** 2).sum(axis=1) / (r.cand_variance[0] + r.noise[0])
    f2 = np.max(np.abs(r.reduction[0] - own) / ((300 + 4) * EPS * own))
    a, _, _, deg, Cr, dd = ar.alc(p, cand, ref, w, r.noise[0])
    f3 = np.max(np.abs(r.reduction[0] - a) / ar.alc_bar(p, cand, ref, w, Cr, dd))
    print("%s D=%d: covariance %.3g of the entry bar (largest |c| %.3g), epilogue %.3g of (m_r + 4) eps, ALC %.3g of the propagated bar"
          % (kernel, d, f1, np.max(np.abs(want)), f2, f3))
    assert f1 <= 1. and f2 <= 1. and f3 <= 1. and not deg.any() and not r.degenerate.any()
    assert np.max(np.abs(want)) > 1e3 * np.max(bar)             # the covariance stands far above what the bar resolves
    assert np.array_equal(r.cand_variance[0], gp.predict(cand, include_nugget=False, deriv=False).unc)
    assert _same(r, M.alc_criterion(gp, cand, ref, weights=w, max_points=128))


# ---- 8. ALCDesign ----------------------------------------------------------------------------------------------------------------------------

def _simulator(x):
    return np.sin(3.0 * x[0]) + x[1] * x[1]


def test_alc_design(tmp_path):
    from mogp_emulator_amd import ALCDesign, LatinHypercubeDesign
    LibGPGPU.set_fit_options(seed=11)
    try:
        def run(design, steps):
            picks, ties = [], 0
            for _ in range(steps):
                design.run_next_point()
                gp, cand, ref = design.gp, design.get_candidates(), design.reference
                assert cand.shape == (64, 2) and ref.shape == (100, 2) and design._scores.shape == (64,)
                chosen = int(np.flatnonzero(np.all(cand == design.get_inputs()[-1], axis=1))[0])
                assert chosen == int(np.argmax(design._scores))
                th = np.asarray(gp.theta.get_data())
                p = ar.Posterior(gp.inputs, th, "SquaredExponential", gp.nugget)
                w = np.full(100, .01)
                a, _, _, _, Cr, d = ar.alc(p, cand, ref, w, gp.nugget)
                bar = ar.alc_bar(p, cand, ref, w, Cr, d)
                order = np.argsort(-a)
                tie = a[order[0]] - a[order[1]] <= bar[order[0]] + bar[order[1]]
                ties += int(tie)
                assert chosen == order[0] or (tie and chosen == order[1]), (chosen, order[:3], a[order[:3]], bar[order[:3]])
                picks.append(chosen)
            return picks, ties
        np.random.seed(5)
        ad = ALCDesign(LatinHypercubeDesign(2), f=_simulator, n_init=8, n_cand=64, n_ref=100, nugget=1e-4)
        ad.run_initial_design()
        picks, ties = run(ad, 2)
        ad.save_design(str(tmp_path / "alc.npz"))
        state = np.random.get_state()
        more, t2 = run(ad, 2)
        print("ALCDesign picks %s, %d of 4 steps with the best two scores inside each other's bar" % (picks + more, ties + t2))
        assert ties + t2 <= 1
        assert ad.get_current_iteration() == 12 and ad.get_inputs().shape == (12, 2)
        # a saved and loaded design continues with the same choices
        again = ALCDesign(LatinHypercubeDesign(2), f=_simulator, n_init=8, n_cand=64, n_ref=7, nugget=1e-4)
        again.load_design(str(tmp_path / "alc.npz"))
        assert again.get_n_ref() == 100 and again.get_current_iteration() == 10
        np.random.set_state(state)
        same, _ = run(again, 2)
        assert same == more and np.array_equal(again.get_inputs(), ad.get_inputs())
        batch = ad.get_batch_points(3)
        assert batch.shape == (3, 2) and len(np.unique(batch, axis=0)) == 3 and ad.get_current_iteration() == 12
        assert ad.get_inputs().shape == (15, 2)
    finally:
        LibGPGPU.set_fit_options(seed=0)
