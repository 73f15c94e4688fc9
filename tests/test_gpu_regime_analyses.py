"""The analyses with arithmetic of their own on the MI355X across the hyperparameter range (regime_cases.py): the design of 130 points, the 37
queries, all eleven regimes and `ard` at D = 17, squared exponential and Matern-5/2.  test_gpu_regimes.py holds every path that consumes
kern_val through cov_build or kgen_sweep; the paths here generate kernel entries with code of their own, or have arithmetic that depends
on the hyperparameters:

  1. kinderiv_kernel      entries of k' read through unit vectors (a sum of one product and zeros is the entry itself), at the queries and at
                          the design itself (an exact zero on the diagonal; `twin`: r2 ~ 1e-17, not 0)
  2. the same two         IterativeGP.predict(deriv=True) against the dense derivative; PosteriorPaths.value_and_gradient (130 features, 3
     products, assembled  draws) on the fields the paths hold
  3. rff_kernel,          the feature product and its input derivative at the staged queries: arguments of 1e2 (`tail`) to 1e9 (`needle`)
     rff_inderiv_kernel
  4. alc_cross_kernel,    predict_cov and alc_criterion: the far sets (translated by 300 correlation lengths: the cross covariance with the
     alc_finish_kernel    design is an exact zero, so the result is the epilogue's generated sigma^2 k alone, held per entry), the general
                          case, and `needle` in closed form
  5. alc_condition_kernel, alc_argmax_kernel      alc_batch, q = 6: picks, every step's scores, the stopping rule at a score of exactly 0
  6. kvar_kernel,         variance_cache / variance_bound at ranks 32 and 130: K ~ sigma^2 I (no pivot order), K ~ sigma^2 1 1^T (rank 1),
     tri_right_kernel     sigma^2 << eta
  7. mixture kernels,     predict_marginal over the ten regimes of the shared design as samples of one emulator; sample_posterior with
     sample kernels       Sigma~ = (sigma^2 + eta) I, ~ eta I and of order e^+-18

Every reference is long double or a float64 restatement whose distance from long double test_regime_analyses_host.py shows; the bars are

  entries of k'           regime_cases.deriv_entries: 2^-52 (FIXED_ULPS_DR2 + (D + 1) gain') |want| per entry, and the subnormal steps carried
                          through the later factors (derived there)
  feature product         pathwise_restate.rff_bar, inputderiv_restate.rffgrad_bar
  far entries             regime_cases.entry_bar, as test_gpu_regimes.py holds generated entries
  predict_cov, ALC        alc_restate.Posterior.cov_bar, alc_restate.alc_bar against the long-double Posterior
  alc_batch               alc_restate.alc_bar of the posterior of the design and the device's own earlier picks (float64, LAPACK), as
                          test_gpu_alc_batch.py; a pick is pinned at every step before the first whose top-two gap is below 20 bars
  d mean / dx, paths      regime_cases.deriv_bar, regime_cases.path_truth: the bars of test_gpu_inputderiv.py and test_gpu_pathwise.py
  variance bound          regime_cases.bound_cache: the bars of test_gpu_variance_bound.py, on the device's own pivots
  mixture, joint draws    100 x the float64 / long double disagreement of marginal_restate.mixture; test_gpu_sample.py's derived bound

Every figure is printed as a fraction of its bar (pytest -s); DESIGN.md section 4 "The analyses across the hyperparameter range" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.LocalGP import _KERNELS
from mogp_emulator_amd.Priors import GPPriors

import regime_cases as rc
from regime_cases import LD
from regime_cases import GAP, TIGHT

pytestmark = pytest.mark.gpu
CASES = pytest.mark.parametrize("case", rc.cases(), ids=lambda c: "%s-%s-D%d" % c)
BATCH_CASES = pytest.mark.parametrize("case", [c for c in rc.cases() if c[0] != "needle"], ids=lambda c: "%s-%s-D%d" % c)
NUGGETS = pytest.mark.parametrize("fit", [False, True], ids=["fixed", "fit"])
EPS = rc.EPS


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _gp(r, fit):
    gp = M.GaussianProcessGPU(r.X, r.t, kernel=r.kernel, nugget="fit" if fit else r.nugget,
                              priors=GPPriors(n_corr=r.X.shape[1], nugget_type="fit" if fit else "fixed"))
    gp.fit(rc.theta(r, fit))
    return gp


def _report(what, fracs):
    print("regime %s: %s" % (what, ", ".join("%s %.3g" % kv for kv in fracs.items())), flush=True)
    bad = {k: v for k, v in fracs.items() if not v <= 1.}
    assert not bad, "%s: beyond the bar (fractions of it): %s" % (what, bad)


def _native(r):
    return LibGPGPU.LocalGP_GPU(r.X, r.t[None, :])


# ---- 1. entries of k' ------------------------------------------------------------------------------------------------------------------------
@CASES
def test_entries_of_the_kernel_derivative(case):
    name, kernel, D = case
    r = rc.regime(*case)
    kt, h = _KERNELS[kernel][0], _native(r)
    eye = np.eye(rc.N)
    got_q = h.kmatvec_inputderiv(kt, rc.scales(r), rc.sigma2(r), eye, r.Xs)
    got_x = h.kmatvec_inputderiv(kt, rc.scales(r), rc.sigma2(r), eye, r.X)
    h.close()
    fracs = {}
    for tag, got, on_design in (("queries", got_q, False), ("design", got_x, True)):
        want, bar, literal = rc.deriv_entries(*case, on_design)
        assert got.shape == want.shape and np.all(np.isfinite(got))
        if on_design:
            i = np.arange(rc.N)
            assert np.all(got[i, :, i] == 0.), "r2 = 0 and a zero difference: the diagonal must be exact zeros"
        if name == "needle":
            assert not got.any(), "a needle's entries must be exact zeros"
        fracs[tag] = rc.excess(got, want, bar)
        sub = np.abs(want) < LD(rc.TINY)
        print("%s: %d entries below the smallest normal double, %d of them non-zero on the device; %.3g of the literal bar of two subnormal steps"
              % (tag, int(sub.sum()), int(np.sum(sub & (got != 0.))), rc.excess(got, want, literal)))
        if (name, kernel) == ("underflow", "SquaredExponential"):
            assert np.any(sub & (got != 0.))                       # gradual underflow: the subnormal results are there
    if name == "twin":
        assert got_x[0, 0, rc.N - 1] != 0. and got_x[rc.N - 1, 0, 0] == -got_x[0, 0, rc.N - 1]
    _report("%s %s D=%d entries of k'" % case, fracs)


# ---- 3. the feature product ------------------------------------------------------------------------------------------------------------------
@CASES
def test_feature_product_and_its_derivative_at_large_arguments(case):
    r, fr = rc.regime(*case), rc.feature_reference(*case)
    h = _native(r)
    val = h.rff(rc.scales(r), fr["omega"], fr["phase"], fr["W"], fr["amp"], queries=r.Xs)
    grad = h.rff_inputderiv(rc.scales(r), fr["omega"], fr["phase"], fr["W"], fr["amp"], r.Xs)
    h.close()
    assert val.shape == (rc.PATH_S, rc.M) and grad.shape == (rc.PATH_S, rc.M, case[2]) and np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    print("largest |argument| %.3g" % fr["arg"])
    _report("%s %s D=%d features" % case, {"value": rc.excess(val.T, fr["val"], fr["vbar"]),
                                           "derivative": rc.excess(np.transpose(grad, (1, 2, 0)), fr["grad"], fr["gbar"])})


# ---- 4. predict_cov and alc_criterion ---------------------------------------------------------------------------------------------------------
@NUGGETS
@CASES
def test_far_sets_give_the_epilogues_generated_entries_alone(case, fit):
    """k between the far sets and the design is an exact zero (past both clamps of exp_dev.h), hence V = L^-1 0 = 0 and the result is
    fl(sigma^2 k) of the epilogue, whatever the factor"""
    name, kernel, D = case
    r, ps, far = rc.regime(*case), rc.point_sets(*case), rc.far_reference(*case)
    gp, s2 = _gp(r, fit), rc.sigma2(r)
    ab, aa = M.predict_cov(gp, ps["far_a"], ps["far_b"])[0], M.predict_cov(gp, ps["far_a"])[0]
    assert np.all(np.isfinite(ab)) and np.all(ab >= 0.) and np.all(np.isfinite(aa)) and np.all(aa >= 0.)
    assert np.all(np.diag(aa) == s2), "the diagonal is not sigma^2 to the bit"
    off = ~np.eye(rc.M, dtype=bool)
    if name == "needle":
        assert not ab.any() and not aa[off].any()
    fracs = {"far_a x far_b": rc.entry_excess(ab, *far["ab"], kernel, D),
             "far_a x far_a": rc.entry_excess(np.where(off, aa, 0.), np.where(off, far["aa"][0], LD(0)), far["aa"][1], kernel, D)}
    for tag in ("far_a", "far_b"):
        res = M.alc_criterion(gp, ps[tag], ps["ref"], noise=r.nugget)
        assert np.all(res.cand_variance == s2), "%s: s^2 of a far candidate is not sigma^2 to the bit" % tag
        assert not res.degenerate.any() and np.all(np.isfinite(res.reduction)) and np.all(res.reduction >= 0.)
    _report("%s %s D=%d far sets %s" % (*case, "fit" if fit else "fixed"), fracs)


@NUGGETS
@CASES
def test_predict_cov_and_alc_against_the_long_double_posterior(case, fit):
    name, kernel, D = case
    r, ps, ref = rc.regime(*case), rc.point_sets(*case), rc.alc_reference(*case)
    gp = _gp(r, fit)
    C = M.predict_cov(gp, ps["cand"], ps["ref"])[0]
    res = M.alc_criterion(gp, ps["cand"], ps["ref"], noise=r.nugget)
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(res.reduction)) and np.all(res.reduction >= 0.) and res.noise[0] == r.nugget
    assert not res.degenerate.any() and not ref["deg"].any()
    assert np.array_equal(res.cand_variance[0], gp.predict(ps["cand"], include_nugget=False, deriv=False).unc)
    assert np.array_equal(res.ref_variance[0], gp.predict(ps["ref"], include_nugget=False, deriv=False).unc)
    _report("%s %s D=%d ALC %s" % (*case, "fit" if fit else "fixed"),
            {"predict_cov": rc.excess(C, ref["C"], ref["cbar"]), "alc_criterion": rc.excess(res.reduction[0], ref["alc"], ref["abar"])})


@NUGGETS
@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_needle_alc_in_closed_form(kernel, fit):
    """K = sigma^2 I and k(x, X) = 0: c(r_j, c_i) is sigma^2 where the two are one point and 0 elsewhere, so with the first five reference
    points appended to the candidates ALC is w_j sigma^4 / (sigma^2 + tau) for those five -- three roundings, held to 4 ulps -- and exactly 0
    for the rest"""
    r, ps = rc.regime("needle", kernel), rc.point_sets("needle", kernel)
    gp, s2 = _gp(r, fit), rc.sigma2(r)
    cand = np.vstack([ps["cand"], ps["ref"][:rc.N_SHARED]])
    res = M.alc_criterion(gp, cand, ps["ref"], noise=r.nugget)
    want = LD(1) / LD(rc.N_REF) * LD(s2) * LD(s2) / (LD(s2) + LD(r.nugget))
    assert not res.degenerate.any() and not res.reduction[0, :rc.N_CAND].any()
    err = float(np.max(np.abs(res.reduction[0, rc.N_CAND:].astype(LD) - want) / (LD(EPS) * want)))
    _report("needle %s closed form %s" % (kernel, "fit" if fit else "fixed"), {"the five shared points (of 4 ulps)": err / 4.})


# ---- 5. alc_batch ----------------------------------------------------------------------------------------------------------------------------
@BATCH_CASES
def test_greedy_batches(case):
    """every regime but `needle`, whose scores are exact zeros (no gap to speak of): test_needle_batches_stop_at_a_score_of_zero"""
    name, kernel, D = case
    r, ps, g = rc.regime(*case), rc.point_sets(*case), rc.batch_reference(*case)
    q = rc.BATCH_Q
    res = M.alc_batch(_gp(r, False), ps["cand"], ps["ref"], q, noise=r.nugget)
    picks = res.picks[0]
    below = np.flatnonzero(g["gap"][0] < GAP)
    t0 = int(below[0]) if below.size else q
    if name in TIGHT:
        assert t0 == q
    print("picks %s, the restatement's %s, top-two gaps %s bars: pinned before step %d" % (picks, g["picks"][0], np.array2string(g["gap"][0], precision=3), t0))
    assert np.array_equal(picks[:t0], g["picks"][0, :t0]) and res.n_picked[0] == q and np.all(picks >= 0) and len(set(picks.tolist())) == q
    assert not res.degenerate.any() and np.all(np.isfinite(res.reduction)) and np.all(res.pending_skipped == 0)
    steps = rc.batch_steps(*case, tuple(int(i) for i in picks))             # the fresh route on the device's own history: no step uncompared
    frac = float(np.max(np.abs(res.reduction[0] - steps["alc"]) / steps["bar"]))
    pb = steps["bar"][np.arange(q), picks]
    tol = steps["iv_bar"][0] + np.concatenate([[0.], np.cumsum(pb)]) + steps["iv_bar"]
    fiv = float(np.max(np.abs(res.integrated_variance[0] - steps["iv"]) / tol))
    # an unpinned pick is still a best candidate to within the two bars
    mask, late = np.zeros(rc.N_CAND, dtype=bool), 0.
    for t in range(q):
        a = np.where(mask, -np.inf, steps["alc"][t])
        best = int(np.argmax(a))
        late = max(late, float((a[best] - a[picks[t]]) / (steps["bar"][t, best] + steps["bar"][t, picks[t]])))
        mask[picks[t]] = True
    assert np.array_equal(res.pick_reduction[0], res.reduction[0, np.arange(q), picks])
    _report("%s %s D=%d batch" % case, {"reduction": frac, "integrated variance": fiv, "best score less the pick's (of both bars)": late})


@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_needle_batches_stop_at_a_score_of_zero(kernel):
    r, ps = rc.regime("needle", kernel), rc.point_sets("needle", kernel)
    gp, q = _gp(r, False), rc.BATCH_Q
    res = M.alc_batch(gp, ps["cand"], ps["ref"], q, noise=r.nugget)
    assert np.all(res.picks == -1) and res.n_picked[0] == 0 and not res.reduction.any() and not res.pick_reduction.any()
    assert np.all(res.integrated_variance == res.integrated_variance[0, 0]) and not res.degenerate.any()
    assert np.array_equal(res.ref_variance_after, res.ref_variance)
    # with the five shared points appended: equal scores, lowest index first, then nothing left to gain
    cand = np.vstack([ps["cand"], ps["ref"][:rc.N_SHARED]])
    res = M.alc_batch(gp, cand, ps["ref"], q, noise=r.nugget)
    assert np.array_equal(res.picks[0], np.r_[rc.N_CAND + np.arange(rc.N_SHARED), -1]) and res.n_picked[0] == rc.N_SHARED
    s2 = rc.sigma2(r)
    want = LD(1) / LD(rc.N_REF) * LD(s2) * LD(s2) / (LD(s2) + LD(r.nugget))
    err = float(np.max(np.abs(res.pick_reduction[0, :rc.N_SHARED].astype(LD) - want) / (LD(EPS) * want)))
    assert res.pick_reduction[0, rc.N_SHARED] == 0. and not res.reduction[0, :, :rc.N_CAND].any()
    _report("needle %s batch" % kernel, {"the five picks' reductions (of 4 ulps)": err / 4.})


# ---- 2. the mean's derivative and the paths at large designs -----------------------------------------------------------------------------------
def _iterative(r):
    return M.IterativeGP(_gp(r, False), r.X, r.t, precond_rank=rc.ITER_RANK, rtol=rc.ITER_RTOL, max_iter=rc.ITER_MAX)


@CASES
def test_iterative_mean_derivative_against_the_dense_reference(case):
    """IterativeGP.predict(deriv=True) (kinderiv_kernel at V = alpha) against the long-double dense derivative, at the bar of
    test_gpu_inputderiv.py with the term for the device's own alpha (regime_cases.deriv_bar)"""
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    ig = _iterative(r)
    pr = ig.predict(r.Xs, deriv=True)
    alpha = ig.weights()
    ig.close()
    assert bool(pr.converged) and pr.deriv.shape == (rc.M, case[2]) and np.all(np.isfinite(pr.deriv))
    print("alpha in %s iterations, residual %.3g" % (pr.iterations, pr.residual))
    if case[0] == "needle":
        assert not pr.deriv.any()                                       # k' = 0 everywhere: exact zeros
    _report("%s %s D=%d iterative derivative" % case, {"d mean / dx": rc.excess(pr.deriv, ref["deriv"], rc.deriv_bar(ref, r, alpha, *case))})


@CASES
def test_path_value_and_gradient_on_the_paths_own_fields(case):
    """PosteriorPaths.value_and_gradient, F = 130 features (three staged tiles, the last partial), S = 3 draws with the caller's normals,
    against pathwise_restate / inputderiv_restate in long double on the frequencies, phases, weights and update the object holds"""
    r = rc.regime(*case)
    W, eps = rc.path_normals()
    ig = _iterative(r)
    paths = ig.sample_paths(rc.PATH_S, n_features=rc.PATH_F, seed=rc.PATH_SEED, stream=rc.PATH_STREAM, feature_normals=W, noise_normals=eps)
    val, grad = paths.value_and_gradient(r.Xs)
    ig.close()
    assert paths.converged.all() and val.shape == (rc.PATH_S, rc.M) and grad.shape == (rc.PATH_S, rc.M, case[2])
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and np.array_equal(paths.feature_normals, W)
    v80, vbar, g80, gbar = rc.path_truth(r, paths.omega, paths.phase, paths.feature_normals, paths.update)
    print("residuals %s, iterations %s" % (paths.residual, paths.iterations.tolist()))
    _report("%s %s D=%d paths" % case, {"value": rc.excess(val, v80, vbar), "gradient": rc.excess(grad, g80, gbar)})


# ---- 7. mixtures and joint draws -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", rc.MIX_WEIGHTS)
@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_mixture_over_the_regimes_as_samples_of_one_emulator(kernel, wkind):
    """predict_marginal with caller weights (no importance weights: the log-posteriors differ by thousands and the mixture would be one
    sample) over the ten regimes of the shared design as hyperparameter samples: retarget between samples e^36 apart in sigma^2 and in
    the nugget, and the pivot subtraction of `between`"""
    r = rc.regime("base", kernel)
    a, bars, dis = rc.mixture_reference(kernel, wkind)
    thetas, w = rc.mixture_thetas(kernel), rc.mixture_weights(wkind)
    gp = _gp(r, True)
    res = M.predict_marginal(gp, r.Xs, thetas=thetas, weights=w)
    assert res.ok.all() and max(dis.values()) <= rc.ILL
    fracs = {}
    for q, got in (("mean", res.mean), ("within", res.within), ("between", res.between)):
        assert got.shape == (rc.M,) and np.all(np.isfinite(got))
        fracs[q] = float(np.abs(got - a[q]).max()) / bars[q]
    assert np.all(res.within >= 0.) and np.all(res.between >= 0.) and abs(res.weights.sum() - 1.) < 1e-14
    fracs["log-weights (of 100 x 2^-52)"] = float(np.abs(np.log(res.weights) - np.log(a["weights"])).max()) / (rc.MIX_MARGIN * EPS)
    # the emulator's own fit is what it was
    assert np.array_equal(gp.predict(r.Xs, deriv=False).mean, _gp(r, True).predict(r.Xs, deriv=False).mean)
    _report("%s mixture, %s weights" % (kernel, wkind), fracs)


@CASES
def test_joint_draws_against_the_restatement(case):
    """sample_posterior, m = 37, S = 3, with the nugget: the batched factor of Sigma~, which is (sigma^2 + eta) I in `needle`, 1e-4 I to
    half a digit in `long` and `noise_only`, and of order e^18 and e^-18 in the sigma regimes; no rung of the ladder anywhere
    (test_regime_analyses_host.py).  The bar is test_gpu_sample.py's: 4 m 2^-52 cond_2(Sigma~) max sqrt(S_jj) |z_s|_2 against
    sample_restate.sample on this build's predict(full_cov=True)"""
    import sample_restate as sr
    r = rc.regime(*case)
    gp, z = _gp(r, False), rc.draw_normals()
    p = gp.predict(r.Xs, full_cov=True, include_nugget=False, deriv=False)
    res = M.sample_posterior(gp, r.Xs, z=z)
    assert res.samples.shape == (rc.DRAWS, rc.M) and res.ok is True and res.jitter_used == 0. and np.array_equal(res.mean, p.mean)
    want, ju, ok, St = sr.sample(p.mean, p.unc, z, nugget=r.nugget)
    assert ok and ju == 0.
    bar = 4. * rc.M * EPS * np.linalg.cond(St) * np.sqrt(np.max(np.diag(St))) * np.linalg.norm(z, axis=-1)
    fracs = {"draws": float(np.max(np.max(np.abs(res.samples - want), axis=-1) / bar))}
    if case[0] == "needle":
        s2 = rc.sigma2(r)
        assert not p.mean.any() and np.array_equal(p.unc, s2 * np.eye(rc.M))
        exact = np.sqrt(LD(s2) + LD(r.nugget)) * z.astype(LD)                   # mean + sqrt(sigma^2 + eta) z, the mean an exact 0
        fracs["closed form (of 2 ulps)"] = float(np.max(np.abs(res.samples.astype(LD) - exact) / (2 * LD(EPS) * np.abs(exact))))
    _report("%s %s D=%d joint draws" % case, fracs)


# ---- 6. the variance bound -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", rc.VAR_RANKS)
@CASES
def test_variance_bound_cache_and_bound(case, rank):
    """IterativeGP.variance_cache / variance_bound (the pivoted factor, tri_right_kernel, kvar_kernel) at preconditioner ranks 32 and 130
    against variance_bound_restate on the device's own pivots -- `needle` and `noise_only` have no pivot order to speak of, and a tie
    anywhere else must not decide a comparison either -- and the long-double dense variance: the bound is never below it by more than
    the bar, and equals it to the bar where the cache has all N columns.  Columns of R are compared up to the first one the restatement does
    not determine (regime_cases.bound_cache); R^T A R = I and the two-sided bound hold the others, as in test_gpu_variance_bound.py."""
    import dimension_cases as dc
    import variance_bound_restate as vr
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    K, ks, _ = rc.bound_inputs(*case)
    ig = M.IterativeGP(_gp(r, False), r.X, r.t, precond_rank=rank, rtol=rc.ITER_RTOL, max_iter=rc.ITER_MAX)
    piv = ig.preconditioner()[1]
    R, vrank = ig.variance_cache()
    reached = len(piv)
    assert R.shape == (rc.N, vrank) and 1 <= vrank <= reached <= rank and np.all(np.isfinite(R)) and len(set(piv.tolist())) == reached
    ch, bar, cond, amp, own, first = rc.bound_cache(*case, reached, pivots=tuple(int(i) for i in piv))
    rr = min(vrank, ch.var_rank)
    assert rr >= vrank - 1 and rr >= ch.var_rank - 1, (vrank, ch.var_rank)
    cols = np.array([dc.excess("fullcov", R[:, j], ch.R[:, j], amp) for j in range(rr)])
    # every column before the first that the restatement does not determine over its seven roundings of K is held, in a cache cut by tau as
    # in any other; behind it the figure is printed, and R^T A R = I and the two-sided bound hold the columns
    held = np.arange(rr) < min(first, rr)
    if not held.all():
        print("columns %d .. %d, which the restatement does not determine: at most %.3g bars from it (its own error there up to %.3g)" % (
            first, rr - 1, float(np.max(cols[~held])), float(np.max(own[first:rr]))))
    A = K + r.nugget * np.eye(rc.N)
    got = ig.variance_bound(r.Xs, rank=rr)
    full = ig.variance_bound(r.Xs)
    ig.close()
    assert got.shape == (rc.M,) and np.all(np.isfinite(got)) and np.all(full <= got)
    gap = full - np.asarray(ref["var"], dtype=np.float64)
    print("rank reached %d, var_rank %d (restatement %d), cond(H) %.3g, %d of %d columns held; (bound - dense) / bar in [%.3g, %.3g]" % (
        reached, vrank, ch.var_rank, cond, int(held.sum()), rr, gap.min() / bar, gap.max() / bar))
    fracs = {"columns of R": float(np.max(cols[held])) if held.any() else 0.,
             "R^T A R - I": dc.excess("fullcov", R.T @ A @ R, np.eye(vrank), amp),
             "bound": dc.excess("var", got, vr.bound(ch.R, ks, rc.sigma2(r), r.nugget, rank=rr), amp),
             "dense variance less the bound": float(np.max(-gap)) / bar}
    if vrank == rc.N:
        fracs["bound against the dense variance at rank N"] = float(np.max(np.abs(gap))) / bar
    _report("%s %s D=%d variance bound, rank %d" % (*case, rank), fracs)
