"""Host-side checks of greedy ALC batches: alc_batch_plan (csrc/predict_plan.h) against a hand-worked table through a sanitised host
program, the exports, the refusals that need no device, the arithmetic of ALCBatchResult, ALCDesign.get_conditioned_batch's bookkeeping
with a stubbed alc_batch, and the NumPy restatement (alc_batch_restate.py): its incremental-row route against its fresh factorisations
on the inputs of tests/test_gpu_alc_batch.py -- inside the derived bars and not identical, so the bars the device is held to are not
vacuous -- and its handling of a run noise tau that differs from the nugget."""
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import ActiveLearning, LibGPGPU

import alc_restate as ar
import alc_batch_restate as br
from test_alc_host import _build_and_run, _fake_gp

N, D, E = 130, 3, 3


def test_alc_batch_plan_matches_the_hand_worked_table(tmp_path):
    out = _build_and_run(tmp_path, "alc_batch_plan_check")
    assert out.strip() == "ok 11 rows"


def test_exports():
    assert M.alc_batch is ActiveLearning.alc_batch and M.ALCBatchResult is ActiveLearning.ALCBatchResult
    assert "greedy batches with conditioning" not in ActiveLearning.__doc__
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import ALCDesign, _capi, libgpgpu
        assert callable(ALCDesign.get_conditioned_batch)
        assert hasattr(libgpgpu.DenseGP_GPU, "alc_batch") and hasattr(libgpgpu.MultiOutputGP_GPU, "alc_batch")
        assert "mogp_densegp_alc_batch" in _capi.SIGNATURES and "mogp_mogp_alc_batch" in _capi.SIGNATURES


def test_not_a_gpu_emulator_is_refused():
    X = np.zeros((4, 2))
    for bad in (None, object(), np.zeros(3), "gp"):
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.alc_batch(bad, X, X, 2)


@pytest.mark.skipif(not LibGPGPU.HAVE_LIBGPGPU, reason="the library is not built")
def test_refusals_come_before_any_device_call(monkeypatch):
    gp = _fake_gp(monkeypatch)
    gp._densegp_gpu.alc_batch = gp._densegp_gpu.alc
    X, R = np.random.default_rng(0).random((5, 3)), np.random.default_rng(1).random((7, 3))
    for b in (np.zeros((5, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="must have shape"):
            M.alc_batch(gp, b, R, 1)
        with pytest.raises(ValueError, match="must have shape"):
            M.alc_batch(gp, X, b, 1)
        with pytest.raises(ValueError, match="pending must have shape"):
            M.alc_batch(gp, X, R, 1, pending=b)
    for v in (np.nan, np.inf):
        Xb = X.copy()
        Xb[2, 1] = v
        with pytest.raises(ValueError, match="must be finite"):
            M.alc_batch(gp, Xb, R, 1)
        with pytest.raises(ValueError, match="must be finite"):
            M.alc_batch(gp, X, R, 1, pending=Xb)
        with pytest.raises(ValueError, match="must be finite"):
            M.alc_batch(gp, X, R, 1, weights=np.r_[v, np.ones(6)])
        with pytest.raises(ValueError, match="noise must be a finite number that is not negative"):
            M.alc_batch(gp, X, R, 1, noise=v)
    with pytest.raises(ValueError, match="weights must have shape"):
        M.alc_batch(gp, X, R, 1, weights=np.ones(6))
    with pytest.raises(ValueError, match="weights must not be negative"):
        M.alc_batch(gp, X, R, 1, weights=np.r_[-1e-300, np.ones(6)])
    with pytest.raises(ValueError, match="weights must not sum to 0"):
        M.alc_batch(gp, X, R, 1, weights=np.zeros(7))
    with pytest.raises(ValueError, match="noise must be a finite number that is not negative"):
        M.alc_batch(gp, X, R, 1, noise=-1e-12)
    with pytest.raises(ValueError, match="max_slots and max_points must not be negative"):
        M.alc_batch(gp, X, R, 1, max_slots=-1)
    for q in (0, -3):
        with pytest.raises(ValueError, match="n_points must be at least 1"):
            M.alc_batch(gp, X, R, q)
    with pytest.raises(ValueError, match="n_points must not exceed the number of candidates"):
        M.alc_batch(gp, X, R, 6)
    with pytest.raises(ValueError, match="n_points must not exceed the number of candidates"):
        M.alc_batch(gp, X, R, 6, pending=R)          # pending points are no candidates
    for sel in ("all", None, "Each", 1):
        with pytest.raises(ValueError, match="select must be"):
            M.alc_batch(gp, X, R, 1, select=sel)
    for kw, msg in ((dict(nugget_type="pivot"), 'not available with nugget="pivot"'), (dict(analytic=True), "not available with analytic_mean=True"),
                    (dict(fit=False), "hyperparameters have not been fit")):
        g = _fake_gp(monkeypatch, **kw)
        g._densegp_gpu.alc_batch = g._densegp_gpu.alc
        for sel in ("each", "total"):
            with pytest.raises(RuntimeError, match=msg):
                M.alc_batch(g, X, R, 2, select=sel)
        assert g._densegp_gpu.calls == 0
    assert gp._densegp_gpu.calls == 0
    # and a call that passes every check does reach the native layer
    with pytest.raises(AssertionError, match="the device must not be reached"):
        M.alc_batch(gp, X, R, 5, pending=R[:2])
    assert gp._densegp_gpu.calls == 1


def test_alc_batch_result_arithmetic():
    picks = np.array([[4, 0, -1], [-1, -1, -1], [2, 1, 3]])
    iv = np.array([[3., 2., 1.5, 1.5], [np.nan] * 4, [2., 1., .75, .5]])
    pts = np.zeros((3, 3, 2))
    r = M.ALCBatchResult(picks=picks, emulator_picks=picks, points=pts, pick_reduction=-np.diff(iv, axis=1), reduction=None, degenerate=None,
                         cand_variance=np.zeros((3, 5)), ref_variance=np.zeros((3, 2)), ref_variance_after=np.zeros((3, 2)),
                         integrated_variance=iv, pending_skipped=np.zeros(3, dtype=int), noise=np.zeros(3), weights=np.full(2, .5))
    assert r.n_picked.tolist() == [2, 0, 3]
    tr = r.total_reduction
    assert tr[0] == 1.5 and np.isnan(tr[1]) and tr[2] == 1.5
    assert r.reduction is None and r.degenerate is None


@pytest.mark.skipif(not LibGPGPU.HAVE_LIBGPGPU, reason="the library is not built")
def test_get_conditioned_batch_bookkeeping(monkeypatch):
    from mogp_emulator_amd import ALCDesign, LatinHypercubeDesign
    calls = []

    def fake_batch(gp, candidates, reference, n_points, noise=None, keep_scores=True, **kw):
        calls.append((gp, candidates.shape, reference.shape, n_points, noise, keep_scores, kw))
        picks = np.array([[5, 2, 7, -1][:n_points]])
        pts = np.where((picks >= 0)[..., None], candidates[np.maximum(picks, 0)], np.nan)
        return M.ALCBatchResult(picks=picks, emulator_picks=picks, points=pts, pick_reduction=np.zeros((1, n_points)), reduction=None,
                                degenerate=None, cand_variance=None, ref_variance=None, ref_variance_after=None,
                                integrated_variance=np.zeros((1, n_points + 1)), pending_skipped=np.zeros(1, dtype=int), noise=np.zeros(1),
                                weights=None)
    monkeypatch.setattr(ActiveLearning, "alc_batch", fake_batch)
    fits = []

    def fake_fit(self):
        fits.append(self.inputs.shape[0])
        self.gp = "the fitted emulator"
    monkeypatch.setattr(ALCDesign, "_fit_emulator", fake_fit)
    np.random.seed(4)
    ad = ALCDesign(LatinHypercubeDesign(2), n_init=6, n_cand=9, n_ref=33, nugget=1e-3, noise=.25)
    with pytest.raises(ValueError, match="Initial design has not been generated"):
        ad.get_conditioned_batch(2)
    ad.generate_initial_design()
    ad.set_initial_targets(np.arange(6.))
    batch = ad.get_conditioned_batch(3)
    assert fits == [6] and len(calls) == 1                      # one fit, one call
    gp, cs, rs, q, noise, keep, kw = calls[0]
    assert gp == "the fitted emulator" and cs == (9, 2) and rs == (33, 2) and q == 3 and noise == .25 and keep is False and kw == {}
    cand = ad.get_candidates()
    assert batch.shape == (3, 2) and np.array_equal(batch, cand[[5, 2, 7]])
    assert ad.get_inputs().shape == (9, 2) and np.array_equal(ad.get_inputs()[6:], batch)
    assert ad.get_current_iteration() == 6 and ad.get_targets().shape == (6,)
    with pytest.raises(AssertionError):
        ad.get_conditioned_batch(2)                             # the batch is pending: its targets come first
    with pytest.raises(AssertionError):
        ad.set_batch_targets(np.zeros(2))
    ad.set_batch_targets(np.array([1., 2., 3.]))
    assert ad.get_current_iteration() == 9 and np.array_equal(ad.get_targets()[6:], [1., 2., 3.])
    # a batch that stops early is as long as its picks
    short = ad.get_conditioned_batch(4)
    assert short.shape == (3, 2) and ad.get_inputs().shape == (12, 2) and fits == [6, 9]
    ad.set_batch_targets(np.zeros(3))
    with pytest.raises(AssertionError, match="n_points must be positive"):
        ad.get_conditioned_batch(0)


# ---- the restatement against itself: the shapes and hyperparameters of tests/test_gpu_alc_batch.py -----------------------------------

def _theta(e, fit):
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, D) + 0.05 * e
    return np.concatenate([corr, [0.2 + 0.03 * e], [-4. + 0.1 * e] if fit else []])


@functools.lru_cache(maxsize=None)
def _inputs(mc, mr):
    rng = np.random.default_rng(77 + D)
    X = rng.random((N, D))
    cand, ref = np.random.default_rng(500 + mc).random((mc, D)), np.random.default_rng(1500 + mr).random((mr, D))
    w = np.random.default_rng(9 + mr).random(mr) + .1
    return X, cand, ref, w / w.sum()


@pytest.mark.parametrize("kind", ("SquaredExponential", "Matern52"))
@pytest.mark.parametrize("fit", (False, True), ids=("fixed", "fit"))
def test_incremental_rows_agree_with_fresh_factorisations_and_are_not_identical(kind, fit):
    mc, mr, q = 129, 300, 17
    X, cand, ref, w = _inputs(mc, mr)
    thetas = [_theta(e, fit) for e in range(E)]
    etas = [float(np.exp(th[-1])) if fit else 1e-2 for th in thetas]
    worst = worst_iv = 0.
    for select in ("each", "total"):
        a = br.greedy(X, thetas, kind, etas, cand, ref, w, etas, q, select=select, route="rows")
        assert np.array_equal(a["picks"], a["picks_fresh"])                   # step by step, both routes choose alike
        assert len(set(np.atleast_2d(a["picks"])[0].tolist())) == q          # never the same candidate twice
        frac = np.max(np.abs(a["alc"] - a["alc_fresh"]) / a["bar"])
        fiv = np.max(np.abs(a["iv"] - a["iv_fresh"]) / a["iv_bar"])
        worst, worst_iv = max(worst, frac), max(worst_iv, fiv)
        assert frac <= 1. and fiv <= 1. and not np.array_equal(a["alc"], a["alc_fresh"])
        # the integrated-variance identity: IV_t = IV_{t-1} - ALC_t[pick_t], per emulator, inside the bars of both sides
        picks = a["picks"] if select == "each" else np.tile(a["picks"], (E, 1))
        for e in range(E):
            for t in range(q):
                i = picks[e, t]
                gap = abs(a["iv"][e, t + 1] - (a["iv"][e, t] - a["alc"][e, t, i]))
                assert gap <= a["iv_bar"][e, t] + a["iv_bar"][e, t + 1] + a["bar"][e, t, i]
        print("%s %s %s: smallest top-two gap %.3g bars (first 6 picks: %.3g)" %
              (kind, "fit" if fit else "fixed", select, np.min(a["gap"]), np.min(np.atleast_2d(a["gap"])[:, :6])))
        assert np.min(a["gap"]) > 1.                                         # no step of the reference is a tie
    print("%s %s: incremental rows off the fresh factorisations by at most %.3g of alc_bar, IV by %.3g of its bar" %
          (kind, "fit" if fit else "fixed", worst, worst_iv))


def test_restatement_takes_a_run_noise_that_is_not_the_nugget():
    mc, mr = 40, 50
    X, cand, ref, w = _inputs(mc, mr)
    th, eta, tau = _theta(1, False), 1e-2, .3
    a = br.greedy(X, [th], "Matern52", [eta], cand, ref, w, [tau], 2, route="fresh")
    b = br.greedy(X, [th], "Matern52", [eta], cand, ref, w, [tau], 2, route="rows")
    assert np.array_equal(a["alc"], b["alc_fresh"]) and np.array_equal(b["picks"], b["picks_fresh"])
    same = br.greedy(X, [th], "Matern52", [eta], cand, ref, w, [eta], 2, route="fresh")
    assert np.array_equal(a["picks"], b["picks"]) and np.max(np.abs(a["alc"] - b["alc"]) / a["bar"]) <= 1.
    # the appended diagonal carries tau, the base rows eta
    Q = a["posts"][0].Q
    assert Q.shape == (N + 2, N + 2)
    sig2 = float(np.exp(th[D]))
    assert abs(Q[0, 0] - (sig2 + eta)) <= 4 * ar.EPS * sig2 and abs(Q[N, N] - (sig2 + tau)) <= 4 * ar.EPS * sig2
    assert abs(Q[N + 1, N + 1] - (sig2 + tau)) <= 4 * ar.EPS * sig2
    # a noisier run removes less variance: step 0 scores differ by the factor (s^2 + eta) / (s^2 + tau) < 1 per candidate
    sc = ar.Posterior(X, th, "Matern52", eta).var(cand)
    np.testing.assert_allclose(a["alc"][0, 0] * (sc + tau), same["alc"][0, 0] * (sc + eta), rtol=1e-12)
    assert a["iv"][0, 0] == same["iv"][0, 0] and a["iv"][0, 1] > same["iv"][0, 1]
    # the definition: after the pick, the variance at the reference points is that of the design with the pick appended at noise tau
    i = a["picks"][0, 0]
    direct = br.Augmented(X, th, "Matern52", eta, cand[i:i + 1], tau).var(ref) @ w
    assert abs(direct - b["iv"][0, 1]) <= a["iv_bar"][0, 1] and direct != b["iv"][0, 1]
    # pending points are a forced prefix: the batch after them is the batch of the design that holds them
    pend = cand[[7, 3]]
    c = br.greedy(X, [th], "Matern52", [eta], cand, ref, w, [tau], 2, pending=pend, route="rows")
    d = br.greedy(X, [th], "Matern52", [eta], cand, ref, w, [tau], 2, pending=pend, route="fresh")
    assert np.array_equal(c["picks"], d["picks"]) and np.max(np.abs(c["alc"] - d["alc"]) / d["bar"]) <= 1.
    assert c["alc"].shape == (1, 2, mc) and c["iv"].shape == (1, 3)
