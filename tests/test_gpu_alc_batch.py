"""Greedy ALC batches on the MI355X (mogp_emulator_amd.ActiveLearning.alc_batch, csrc/kernels_alc.hip) on the data, hyperparameters and
point sets of test_gpu_alc.py: n = 130, D = 3, E = 3, squared exponential and Matern-5/2, fitted and fixed nugget, (m_c, m_r) in
{(129, 300), (300, 129)}, q in {1, 6, 17} (17 crosses a 16-row step of the product's K range).

The reference is alc_batch_restate.py: after every pick the design with the picked points appended (noise tau on their diagonal) is
factored afresh, and the criterion and its bars are alc_restate's.  Every bar is derived, none is measured:
    a step's reduction      alc_restate.alc_bar of the posterior of X u picks
    the integrated variance var_bar(ref) @ w of the posterior the chain starts from, plus the bars of the reductions subtracted since
    a pick                  must equal the reference's exactly, and the reference's best two scores must lie further apart than the sum
                            of their bars at every step (no ties), which is asserted here on the CPU
Measured figures are printed as fractions of their bars; DESIGN.md section 3 "Active learning: batches" records them.
"""
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import alc_restate as ar
import alc_batch_restate as br
from test_gpu_alc import MODELS, D, E, N, _cand, _data, _eta, _kind, _model, _model_id, _points, _ref, _single, _theta, _weights

pytestmark = pytest.mark.gpu
EPS = 2. ** -52
SHAPES = ((129, 300), (300, 129))
QS = (1, 6, 17)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


@functools.lru_cache(maxsize=None)
def _greedy(kernel, nugget, mc, mr, select, tau=None, q=max(QS)):
    """the restatement's batch of q picks for the three emulators; computed once, never modified"""
    fit = nugget == "fit"
    etas = [_eta(nugget, e) for e in range(E)]
    taus = etas if tau is None else [tau] * E
    return br.greedy(_data()[0], [_theta(e, fit) for e in range(E)], kernel, etas, _cand(mc), _ref(mr), _weights(mr), taus, q, select=select)


def _same(a, b):
    eq = lambda x, y: (x is None and y is None) or np.array_equal(x, y, equal_nan=True)
    return all(eq(getattr(a, k), getattr(b, k)) for k in ("picks", "emulator_picks", "points", "pick_reduction", "reduction", "degenerate",
                                                         "cand_variance", "ref_variance", "ref_variance_after", "integrated_variance",
                                                         "pending_skipped", "noise"))


# ---- 1. step 0 is alc_criterion ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_step_0_is_alc_criterion(mk):
    mo = _model(*mk)
    for mc, mr in SHAPES:
        cand, ref, w = _cand(mc), _ref(mr), _weights(mr)
        a = M.alc_criterion(mo, cand, ref, weights=w)
        for select in ("each", "total"):
            r = M.alc_batch(mo, cand, ref, 1, weights=w, select=select)
            assert r.reduction.shape == (E, 1, mc) and r.degenerate.shape == (E, 1, mc) and r.degenerate.dtype == bool
            assert np.array_equal(r.reduction[:, 0], a.reduction) and np.array_equal(r.degenerate[:, 0], a.degenerate)
            assert np.array_equal(r.cand_variance, a.cand_variance) and np.array_equal(r.ref_variance, a.ref_variance)
            assert np.array_equal(r.noise, a.noise) and np.array_equal(r.weights, w)
            np.testing.assert_allclose(r.integrated_variance[:, 0], a.integrated_variance, rtol=(mr + 4) * EPS)
            if select == "each":
                assert r.picks.shape == (E, 1) and np.array_equal(r.picks[:, 0], a.best)
                assert np.array_equal(r.pick_reduction[:, 0], a.reduction[np.arange(E), a.best])
            else:
                # the host's sum: ascending emulators, each row divided by its own integrated variance
                total = sum(a.reduction[e] / r.integrated_variance[e, 0] for e in range(E))
                assert r.picks.shape == (1,) and r.picks[0] == int(np.argmax(total))
            assert np.array_equal(r.integrated_variance[:, 1], r.integrated_variance[:, 0] - r.pick_reduction[:, 0])
            assert np.array_equal(r.points, cand[r.picks]) and np.array_equal(r.n_picked, np.ones(E))


# ---- 2. picks and every step's scores against the restatement ------------------------------------------------------------------------------

def _against_restatement(mo, g, cand, ref, w, q, select, noise=None):
    """asserts the picks, every step's reduction and the integrated variances of one device call against the restatement g; returns the
    largest fractions of the bars (reduction, integrated variance)"""
    r = M.alc_batch(mo, cand, ref, q, weights=w, select=select, noise=noise)
    assert np.array_equal(r.picks, g["picks"][..., :q]), (r.picks, g["picks"][..., :q])
    assert np.all(r.emulator_picks == (r.picks if select == "each" else r.picks[None, :])) and np.all(r.n_picked == q)
    assert np.all(r.pending_skipped == 0) and not r.degenerate.any() and np.all(np.isfinite(r.reduction))
    frac = np.max(np.abs(r.reduction - g["alc"][:, :q]) / g["bar"][:, :q])
    assert frac <= 1., frac
    ep = r.emulator_picks
    for e in range(E):
        assert np.array_equal(r.pick_reduction[e], r.reduction[e, np.arange(q), ep[e]])
    # IV_t = IV_0 - the reductions of the picks: the bar of IV_0 plus those of the reductions, against the restatement's own bar
    pb = np.take_along_axis(g["bar"][:, :q], ep[:, :, None], axis=2)[:, :, 0]
    tol = g["iv_bar"][:, :1] + np.concatenate([np.zeros((E, 1)), np.cumsum(pb, axis=1)], axis=1) + g["iv_bar"][:, :q + 1]
    fiv = np.max(np.abs(r.integrated_variance - g["iv"][:, :q + 1]) / tol)
    assert fiv <= 1., fiv
    after = r.ref_variance_after @ w
    assert np.all(np.abs(after - g["iv"][:, q]) <= tol[:, q])
    assert np.all(r.ref_variance_after <= r.ref_variance) and np.all(r.ref_variance_after >= 0.)
    return frac, fiv


@pytest.mark.parametrize("select", ("each", "total"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_picks_and_scores_against_the_restatement(mk, shape, select):
    mc, mr = shape
    g = _greedy(*mk, mc, mr, select)
    # the reference's own best two scores are no tie at any step
    assert np.min(g["gap"]) > 1., np.min(g["gap"])
    worst = worst_iv = 0.
    for q in QS:
        frac, fiv = _against_restatement(_model(*mk), g, _cand(mc), _ref(mr), _weights(mr), q, select)
        worst, worst_iv = max(worst, frac), max(worst_iv, fiv)
    print("%s %d x %d %s: reduction off the posterior of X u picks by at most %.3g of alc_bar, IV by %.3g of its bar; smallest top-two "
          "gap of the reference %.3g bars" % (_model_id(mk), mc, mr, select, worst, worst_iv, np.min(g["gap"])))


@pytest.mark.parametrize("select", ("each", "total"))
def test_run_noise_that_is_not_the_nugget(select):
    mk, (mc, mr), tau = MODELS[3], SHAPES[0], .05
    g = _greedy(*mk, mc, mr, select, tau=tau)
    assert np.min(g["gap"]) > 1., np.min(g["gap"])
    frac, fiv = _against_restatement(_model(*mk), g, _cand(mc), _ref(mr), _weights(mr), max(QS), select, noise=tau)
    print("%s tau = %g %s: reduction %.3g of alc_bar, IV %.3g of its bar; smallest top-two gap %.3g bars" %
          (_model_id(mk), tau, select, frac, fiv, np.min(g["gap"])))
    other = _greedy(*mk, mc, mr, select)
    assert not np.array_equal(g["picks"], other["picks"]) or not np.array_equal(g["alc"], other["alc"])


# ---- 3. end to end: a second emulator that holds the picks -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_a_second_emulator_with_the_picks_appended(mk):
    kernel, nugget = mk
    e, q = 1, 6
    gp = _single(kernel, nugget, e)
    cand, ref, w = _cand(129), _ref(300), _weights(300)
    r = M.alc_batch(gp, cand, ref, q + 1, weights=w)             # tau = the nugget of the fit = eta; step q is scored after q picks
    short = M.alc_batch(gp, cand, ref, q, weights=w)
    assert np.array_equal(short.picks, r.picks[:, :q]) and np.array_equal(short.reduction, r.reduction[:, :q])
    assert np.array_equal(short.integrated_variance, r.integrated_variance[:, :q + 1])
    X, T = _data()
    th, eta = _theta(e, nugget == "fit"), _eta(nugget, e)
    Xp = np.vstack([X, r.points[0, :q]])
    g2 = M.GaussianProcessGPU(Xp, np.r_[T[e], np.full(q, .37)], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)))
    g2.fit(th)
    p2 = br.Augmented(X, th, kernel, eta, r.points[0, :q], eta)
    a2 = M.alc_criterion(g2, cand, ref, weights=w)
    _, _, _, _, C, d = ar.alc(p2, cand, ref, w, eta)
    bar = ar.alc_bar(p2, cand, ref, w, C, d)
    f1 = np.max(np.abs(a2.reduction[0] - r.reduction[0, q]) / (2. * bar))
    # the chain of q subtractions against one prediction of the refitted emulator
    p0 = ar.Posterior(X, th, kernel, eta)
    chain = p0.var_bar(ref) @ w
    for t in range(q):
        pt = br.Augmented(X, th, kernel, eta, r.points[0, :t], eta)
        _, _, _, _, Ct, dt = ar.alc(pt, cand, ref, w, eta)
        chain += ar.alc_bar(pt, cand, ref, w, Ct, dt)[r.picks[0, t]]
    tol = chain + p2.var_bar(ref) @ w
    direct = g2.predict(ref, include_nugget=False, deriv=False).unc @ w
    f2 = abs(direct - r.integrated_variance[0, q]) / tol
    f3 = abs(direct - short.ref_variance_after[0] @ w) / tol
    print("%s: alc_criterion of the refitted emulator against step %d: %.3g of both bars; predict(ref).unc @ w against IV_q %.3g and against "
          "ref_variance_after @ w %.3g of the propagated bar; the batch removes %.3g of IV_0" %
          (_model_id(mk), q, f1, f2, f3, short.total_reduction[0] / short.integrated_variance[0, 0]))
    assert f1 <= 1. and f2 <= 1. and f3 <= 1.


# ---- 4. pending points ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("select", ("each", "total"))
@pytest.mark.parametrize("mk", (MODELS[0], MODELS[3]), ids=_model_id)
def test_pending_points_are_conditioned_on_first(mk, select):
    kernel, nugget = mk
    fit = nugget == "fit"
    mo = _model(*mk)
    cand, ref, w, q = _cand(129), _ref(300), _weights(300), 4
    Xp = _points(3, 7)
    r = M.alc_batch(mo, cand, ref, q, weights=w, pending=Xp, select=select)
    assert np.all(r.pending_skipped == 0) and np.all(r.n_picked == q)
    base = M.alc_criterion(mo, cand, ref, weights=w)
    assert np.array_equal(r.cand_variance, base.cand_variance) and np.array_equal(r.ref_variance, base.ref_variance)
    # the restatement with the pending points as a forced prefix
    etas = [_eta(nugget, e) for e in range(E)]
    g = br.greedy(_data()[0], [_theta(e, fit) for e in range(E)], kernel, etas, cand, ref, w, etas, q, pending=Xp, select=select)
    assert np.min(g["gap"]) > 1. and np.array_equal(r.picks, g["picks"])
    f1 = np.max(np.abs(r.reduction - g["alc"]) / g["bar"])
    # the model that holds the pending points as training points (tau = eta)
    X, T = _data()
    m2 = M.MultiOutputGP_GPU(np.vstack([X, Xp]), np.hstack([T[:E], np.zeros((E, 3))]), kernel=kernel, nugget=nugget,
                             priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)))
    for e in range(E):
        m2.fit_emulator(e, _theta(e, fit))
    r2 = M.alc_batch(m2, cand, ref, q, weights=w, select=select)
    assert np.array_equal(r2.picks, r.picks)
    f2 = np.max(np.abs(r.reduction - r2.reduction) / (2. * g["bar"]))
    f3 = np.max(np.abs(r.integrated_variance - r2.integrated_variance) / (2. * (g["iv_bar"][:, :1] + np.sum(np.max(g["bar"], axis=2), axis=1)[:, None])))
    print("%s %s: with 3 pending points, reduction %.3g of alc_bar off the restatement, %.3g of both bars off the model that holds them, "
          "IV %.3g" % (_model_id(mk), select, f1, f2, f3))
    assert f1 <= 1. and f2 <= 1. and f3 <= 1.
    # the forced prefix at the native layer: the same call spelled out
    nat = mo._mogp_gpu.alc_batch(np.vstack([Xp, cand]), 3, ref, w, q, noise=np.ascontiguousarray(mo._nuggets()), total=select == "total")
    assert np.all(nat["picks"][:, :3] == np.arange(3)) and np.array_equal(nat["red"][:, 3:, 3:], r.reduction)
    assert np.array_equal(nat["iv"][:, 3:], r.integrated_variance)


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_same_bits_whatever_the_cut(mk):
    mo = _model(*mk)
    cand, ref, w, q = _cand(300), _ref(129), _weights(129), 6
    base = M.alc_batch(mo, cand, ref, q, weights=w)
    assert _same(base, M.alc_batch(mo, cand, ref, q, weights=w))
    for ms in (1, 0):
        assert _same(base, M.alc_batch(mo, cand, ref, q, weights=w, max_slots=ms)), ms
    for e in range(E):
        one = M.alc_batch(_single(*mk, e), cand, ref, q, weights=w)
        assert one.picks.shape == (1, q) and np.array_equal(one.picks[0], base.picks[e]) and np.array_equal(one.reduction[0], base.reduction[e])
        assert np.array_equal(one.integrated_variance[0], base.integrated_variance[e]) and np.array_equal(one.ref_variance_after[0], base.ref_variance_after[e])
        assert np.array_equal(one.cand_variance[0], base.cand_variance[e]) and np.array_equal(one.degenerate[0], base.degenerate[e])
    lean = M.alc_batch(mo, cand, ref, q, weights=w, keep_scores=False)
    assert lean.reduction is None and lean.degenerate is None
    assert np.array_equal(lean.picks, base.picks) and np.array_equal(lean.pick_reduction, base.pick_reduction)
    assert np.array_equal(lean.integrated_variance, base.integrated_variance) and np.array_equal(lean.ref_variance_after, base.ref_variance_after)
    tot = M.alc_batch(mo, cand, ref, q, weights=w, select="total")
    assert _same(tot, M.alc_batch(mo, cand, ref, q, weights=w, select="total"))
    lt = M.alc_batch(mo, cand, ref, q, weights=w, select="total", keep_scores=False)
    assert np.array_equal(lt.picks, tot.picks) and np.array_equal(lt.pick_reduction, tot.pick_reduction)
    # one emulator: its total batch is its own batch
    s1 = M.alc_batch(_single(*mk, 1), cand, ref, q, weights=w, select="total")
    assert s1.picks.shape == (q,) and np.array_equal(s1.picks, base.picks[1])


@pytest.mark.parametrize("select", ("each", "total"))
def test_same_bits_on_two_parts_of_one_device(select):
    mk = MODELS[1]
    mo, two = _model(*mk), _model(*mk, devices=(0, 0))
    cand, ref, w = _cand(300), _ref(129), _weights(129)
    assert _same(M.alc_batch(mo, cand, ref, 6, weights=w, select=select), M.alc_batch(two, cand, ref, 6, weights=w, select=select))
    assert _same(M.alc_batch(mo, cand, ref, 3, weights=w, select=select, pending=_points(2, 7), keep_scores=False),
                 M.alc_batch(two, cand, ref, 3, weights=w, select=select, pending=_points(2, 7), keep_scores=False))


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------------------

def test_one_candidate_and_a_batch_that_takes_every_candidate():
    mo = _model(*MODELS[0])
    ref = _ref(129)
    for select in ("each", "total"):
        r = M.alc_batch(mo, _cand(1), ref, 1, select=select)
        assert np.all(r.picks == 0) and np.all(r.n_picked == 1) and r.reduction.shape == (E, 1, 1)
        r = M.alc_batch(mo, _cand(300)[:3], ref, 3, select=select)
        assert np.all(np.sort(np.atleast_2d(r.picks), axis=1) == np.arange(3)) and np.all(r.n_picked == 3)
        assert np.all(np.isfinite(r.reduction)) and np.all(np.diff(r.integrated_variance, axis=1) < 0.)
    with pytest.raises(ValueError, match="n_points must not exceed"):
        M.alc_batch(mo, _cand(300)[:3], ref, 4)


def test_nothing_to_gain_stops_the_batch():
    """The setup of test_candidates_on_training_points_without_nugget_are_degenerate: K is the identity to 1e-6, the adaptive nugget stays
    0, and with tau = 0 every candidate on a training point sits at or below the floor: no pick, nothing NaN, nothing raised."""
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[0], nugget="adaptive")
    gp.fit(np.r_[np.full(D, 10.), 0.3])
    assert gp.nugget == 0.
    cand = np.ascontiguousarray(X[:8])
    for select in ("each", "total"):
        r = M.alc_batch(gp, cand, _ref(129), 3, select=select)
        assert r.noise[0] == 0. and np.all(r.n_picked == 0) and np.all(r.picks == -1) and np.all(r.emulator_picks == -1)
        assert np.all(r.degenerate) and np.all(r.reduction == 0.) and np.all(r.pick_reduction == 0.) and np.all(np.isnan(r.points))
        for a in (r.cand_variance, r.ref_variance, r.ref_variance_after, r.integrated_variance):
            assert np.all(np.isfinite(a))
        assert np.array_equal(r.ref_variance_after, r.ref_variance) and np.all(r.integrated_variance == r.integrated_variance[:, :1])
        # a pending point on a training point is skipped and counted
        p = M.alc_batch(gp, _cand(127), _ref(129), 2, pending=X[3:5], select=select)
        assert p.pending_skipped[0] == 2 and np.all(p.n_picked == 2) and np.all(np.isfinite(p.reduction))
        # with noise the same candidates are ordinary ones
        r2 = M.alc_batch(gp, cand, _ref(129), 3, noise=1e-3, select=select)
        assert np.all(r2.n_picked == 3) and not r2.degenerate.any() and np.all(np.isfinite(r2.reduction))
        assert len(set(np.ravel(r2.picks).tolist())) == 3 and np.all(r2.pick_reduction > 0.)


@pytest.mark.parametrize("mk", (MODELS[0], MODELS[3]), ids=_model_id)
def test_partly_fitted_model(mk):
    kernel, nugget = mk
    full, part = _model(*mk), _model(*mk, fit=(0, 2))
    cand, ref, w, q = _cand(300), _ref(129), _weights(129), 3
    a, b = M.alc_batch(full, cand, ref, q, weights=w), M.alc_batch(part, cand, ref, q, weights=w)
    for name in ("reduction", "cand_variance", "ref_variance", "ref_variance_after", "integrated_variance", "pick_reduction"):
        x, y = getattr(a, name), getattr(b, name)
        assert np.all(np.isnan(y[1])) and np.array_equal(x[[0, 2]], y[[0, 2]]), name
    assert np.all(b.picks[1] == -1) and np.array_equal(a.picks[[0, 2]], b.picks[[0, 2]]) and b.n_picked.tolist() == [q, 0, q]
    assert not b.degenerate[1].any() and np.all(np.isnan(b.points[1]))
    # select="total" leaves the emulator that is not fit out of the sum
    t = M.alc_batch(part, cand, ref, q, weights=w, select="total")
    fit = nugget == "fit"
    g = br.greedy(_data()[0], [_theta(e, fit) for e in (0, 2)], kernel, [_eta(nugget, e) for e in (0, 2)], cand, ref, w,
                  [_eta(nugget, e) for e in (0, 2)], q, select="total")
    assert np.min(g["gap"]) > 1. and np.array_equal(t.picks, g["picks"])
    assert np.all(np.isnan(t.reduction[1])) and np.all(t.emulator_picks[1] == -1)
    assert np.max(np.abs(t.reduction[[0, 2]] - g["alc"]) / g["bar"]) <= 1.


# ---- 7. the other kernels, and inputs wider than one slice of dimensions ------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,d", [("SquaredExponential", 80), ("UniformSqExp", 3), ("ProductMat52", 3), ("Matern52", 35)],
                         ids=["D80", "UniformSqExp", "ProductMat52", "D35"])
def test_other_kernels_and_dimensions(kernel, d):
    X, T = _data(N, d)
    nc = ar.n_corr(kernel, d)
    th = _theta(1, False, d, nc)
    if d > 3:
        th[:nc] = np.log(1. / d) + np.linspace(1.5, 3.5, nc)
    gp = M.GaussianProcessGPU(X, T[1], kernel=kernel, nugget=1e-2, priors=GPPriors(n_corr=nc, nugget_type="fixed"))
    gp.fit(th)
    cand, ref, w, q = _points(129, 0, d), _points(300, 1, d), _weights(300), 3
    g = br.greedy(X, [th], kernel, [1e-2], cand, ref, w, [1e-2], q)
    r = M.alc_batch(gp, cand, ref, q, weights=w)
    assert np.min(g["gap"]) > 1. and np.array_equal(r.picks, g["picks"])
    frac = np.max(np.abs(r.reduction - g["alc"]) / g["bar"])
    tol = g["iv_bar"][:, :1] + np.sum(np.max(g["bar"], axis=2), axis=1)[:, None] + g["iv_bar"]
    fiv = np.max(np.abs(r.integrated_variance - g["iv"]) / tol)
    print("%s D=%d: reduction %.3g of alc_bar, IV %.3g of its bar, smallest top-two gap %.3g bars" % (kernel, d, frac, fiv, np.min(g["gap"])))
    assert frac <= 1. and fiv <= 1. and not r.degenerate.any()
    assert np.array_equal(r.reduction[:, 0], M.alc_criterion(gp, cand, ref, weights=w).reduction)


# ---- 8. ALCDesign ----------------------------------------------------------------------------------------------------------------------------------

def _simulator(x):
    return np.sin(3.0 * x[0]) + x[1] * x[1]


def test_alc_design_conditioned_batch():
    from mogp_emulator_amd import ALCDesign, LatinHypercubeDesign
    LibGPGPU.set_fit_options(seed=11)
    try:
        np.random.seed(5)
        ad = ALCDesign(LatinHypercubeDesign(2), f=_simulator, n_init=8, n_cand=64, n_ref=100, nugget=1e-4)
        ad.run_initial_design()
        batch = ad.get_conditioned_batch(3)
        assert batch.shape == (3, 2) and len(np.unique(batch, axis=0)) == 3
        assert ad.get_inputs().shape == (11, 2) and np.array_equal(ad.get_inputs()[8:], batch) and ad.get_current_iteration() == 8
        res = ad.batch_result
        assert np.array_equal(batch, ad.get_candidates()[res.picks[0]]) and ad.reference.shape == (100, 2)
        # the batch is the one a direct call gives, and each pick took something off the integrated variance
        again = M.alc_batch(ad.gp, ad.get_candidates(), ad.reference, 3)
        assert np.array_equal(again.picks, res.picks) and np.all(np.diff(res.integrated_variance[0]) < 0.)
        ad.set_batch_targets(np.array([_simulator(x) for x in batch]))
        assert ad.get_current_iteration() == 11 and ad.get_targets().shape == (11,)
        ad.run_next_point()
        assert ad.get_current_iteration() == 12
    finally:
        LibGPGPU.set_fit_options(seed=0)
