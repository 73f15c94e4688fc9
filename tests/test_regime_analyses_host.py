"""The premises of test_gpu_regime_analyses.py, shown on the CPU: no device here.  For every regime of regime_cases.py and both kernels

  1. entries of k' (regime_cases.deriv_entries): the float64 restatement in the kernel's order lies inside the bar; only `underflow` (squared
     exponential) and `needle` hold entries below the smallest normal double -- 2847 and 14430 of the 14430 entries at the queries, D = 3;
     the literal bar of two subnormal steps is missed by float64 itself in `underflow`, which is why deriv_entries carries the steps;
  3. the feature product and its derivative: the largest argument per regime (1e2 in `tail`, 1e9 in `needle`), float64 within 0.1 of
     rff_bar / rffgrad_bar, and the bars below 1e-4 of amp sum_f |W_f| (the derivative's: of amp s_d sum_f |omega_fd W_f|) even in `needle`: a
     range reduction in less than float64 could not pass;
  4. the far sets: every long-double entry of k between them and the design is below 2^-1080, so the device's cross covariance there is an
     exact zero; alc_bar / ALC below 0.05 in the four tight regimes; the float64 restatement against the long-double one as a fraction of
     both bars;
  5. greedy batches: every top-two gap of tail, underflow, noise_only and big_nugget is at least 20 bars;
  2. float64 paths (value and gradient) lie far inside their bars on their own fields;
  6. the restated variance bound is never below the long-double dense variance by more than its bar; which caches are cut by tau, and up
     to which column the restatement determines the cache (its largest error over seven roundings of K): all of it where nothing is
     cut, a leading part where it is;
  7. the mixture over the regimes disagrees between float64 and long double by less than 1e-8, and which regimes need a rung of the
     jitter ladder for a joint draw at the queries (none does, with the nugget or without).

The share of a bar that float64 itself may take is stated, with its derivation, at each assertion.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import inputderiv_restate as idr
import pathwise_restate as pw
import regime_cases as rc
from regime_cases import LD

from regime_cases import GAP, TIGHT

HALF = 0.5
# (regime, kernel, D) in which float64 may use the whole bar of an entry of k', not half of it, and why:
#   the Matern at gains above 100 (tail, underflow, and ard's short coordinate at D = 3): the bar is its gain term there, (D + 1) g' = 4 g' ulps,
#   and the worst case of the difference-form r2 with t = sqrt(5 r2) is (D / 2 + 2.5) g' = 4 g' ulps at D = 3 -- the whole of it, where the
#   squared exponential's (D / 2 + 1) g' = 2.5 g' leaves 0.63 (measured: 0.51, 0.57 and 0.54 against 0.41 - 0.50 for the squared exponential);
#   underflow, squared exponential: the carried subnormal steps of regime_cases.deriv_entries are the worst case of five roundings, each of
#   which float64 meets in some entry of 14430 (measured: 0.89 at the queries, 0.92 at the design).
WHOLE_BAR = {("tail", "Matern52", 3), ("underflow", "Matern52", 3), ("ard", "Matern52", 3), ("underflow", "SquaredExponential", 3)}


def _ids(c):
    return "%s-%s-D%d" % c


CASES = pytest.mark.parametrize("case", rc.cases(), ids=_ids)


# ---- 1. entries of k' ------------------------------------------------------------------------------------------------------------------------
@CASES
def test_float64_entries_of_the_kernel_derivative_lie_inside_the_bar(case):
    """float64 in the kernel's order lies within half of the bar of every entry, so that the bar is never about the reference; in the four
    cases of WHOLE_BAR within the whole of it, for the reasons given there"""
    name, kernel, D = case
    r = rc.regime(*case)
    s, s2, U = rc.scales(r), rc.sigma2(r), rc.staged(r, r.X)
    for on_design in (False, True):
        want, bar, literal = rc.deriv_entries(*case, on_design)
        Q = U if on_design else rc.staged(r, r.Xs)
        got = idr.kgrad_in(Q, U, s, kernel, s2, np.eye(rc.N))
        frac, lit = rc.excess(got, want, bar), rc.excess(got, want, literal)
        off = np.ones(want.shape, dtype=bool)
        if on_design:
            off[np.arange(rc.N), :, np.arange(rc.N)] = False
            assert np.all(np.asarray(want)[~off] == 0) and np.all(got[~off] == 0.)       # r2 = 0 and a zero difference
        if name != "needle":                                 # an exact zero of the reference is a zero difference (the diagonal; twin's other
            off &= np.asarray(want != 0)                     # coordinates): r2 stays below 1e4 and the long-double exponential above 1e-2000
        sub = int(np.sum((np.abs(want) < LD(rc.TINY)) & off))
        print("%s %s D=%d %s: float64 at %.3g of the bar (%.3g of the literal one), %d of %d entries below the smallest normal double" % (
            *case, "design" if on_design else "queries", frac, lit, sub, int(off.sum())))
        assert frac <= (1. if case in WHOLE_BAR else HALF), (case, frac)
        if name == "needle":
            assert sub == off.sum() and not got.any() and np.all(np.abs(want) < LD(rc.STEP) / 2)
            assert on_design or sub == 14430 or D != 3
        elif (name, kernel) == ("underflow", "SquaredExponential"):
            assert on_design or sub == 2847
            assert lit > 1e3                               # the literal two steps: not what float64 arithmetic in this order can give
        else:
            assert sub == 0 and lit == frac
        if name == "twin" and on_design:
            d0 = np.abs(np.asarray(want[0, 0, rc.N - 1], dtype=np.float64))
            assert 0. < d0 < 1e-7 and got[0, 0, rc.N - 1] != 0.                         # r2 ~ 1e-17, a difference of 1e-9 s: not an exact 0


# ---- 3. the feature product ------------------------------------------------------------------------------------------------------------------
@CASES
def test_feature_bars_hold_float64_and_are_not_vacuous_at_large_arguments(case):
    name, kernel, D = case
    r, fr = rc.regime(*case), rc.feature_reference(*case)
    Pt, s, s2 = rc.staged(r, r.Xs), rc.scales(r), rc.sigma2(r)
    fv = rc.excess(pw.rff(Pt, fr["omega"], fr["phase"], fr["W"], s2), fr["val"], fr["vbar"])
    fg = rc.excess(idr.rff_grad(Pt, s, fr["omega"], fr["phase"], fr["W"], s2), fr["grad"], fr["gbar"])
    vac = float(np.max(fr["vbar"] / fr["scale"][None, :]))
    gscale = fr["amp"] * s[:, None] * (np.abs(fr["omega"]).T @ np.abs(fr["W"]).T)          # (D, S)
    vacg = float(np.max(fr["gbar"] / gscale[None]))
    print("%s %s D=%d: largest |argument| %.3g; float64 at %.3g (value) and %.3g (derivative) of the bars; the bars are %.3g and %.3g of the "
          "largest possible value" % (*case, fr["arg"], fv, fg, vac, vacg))
    assert fv <= 0.1 and fg <= 0.1 and vac <= 1e-4 and vacg <= 1e-4
    if name == "tail":
        assert 50. < fr["arg"] < 500.
    if name == "needle":
        assert 1e8 < fr["arg"] < 1e10


# ---- 4. predict_cov and alc_criterion ---------------------------------------------------------------------------------------------------------
@CASES
def test_far_sets_have_an_exactly_zero_cross_covariance(case):
    r, far, ps = rc.regime(*case), rc.far_reference(*case), rc.point_sets(*case)
    assert ps["cand"].shape == (rc.N_CAND, case[2]) and ps["ref"].shape == (rc.N_REF, case[2]) and np.array_equal(ps["ref"][:rc.M], r.Xs)
    assert ps["far_a"].shape == (rc.M, case[2]) and ps["far_b"].shape == (rc.N_FAR_B, case[2])
    U = rc.staged(r, r.X)
    d = min(float(np.abs(rc.staged(r, ps[k])[:, None, :] - U[None, :, :]).max(axis=2).min()) for k in ("far_a", "far_b"))
    print("%s %s D=%d: largest k between the far sets and the design %s; every pair is at least %.4g scaled units apart in some coordinate" % (*case, far["kstar"], d))
    assert far["kstar"] < LD(2) ** -1080 and d > 240.
    # the entries between the far sets are ordinary ones
    assert float(far["ab"][0].max()) > 1e-3 * rc.sigma2(r) or r.name in ("needle", "underflow", "tail")


@CASES
def test_alc_bars_are_tight_in_four_regimes_and_float64_lies_inside(case):
    """float64 lies within 0.01 of both bars where they are loose (base, long, ard, the sigma regimes, twin: at most 3e-7).  In tail,
    underflow, noise_only and big_nugget cond(Q) is small, the bar of an entry is little more than its absolute part (D + 4) 2^-52 sigma^2
    = 7 ulps of sigma^2, and float64 itself leaves up to an ulp of sigma^2 in an entry (at most 0.16 of the bar measured): there the
    share is 2 / (D + 4), an ulp each for the prior entry and the correction."""
    name, kernel, D = case
    a64, a80 = rc.alc_reference(*case, np.float64), rc.alc_reference(*case)
    fc = float(np.max(np.abs(a64["C"].astype(LD) - a80["C"]) / a80["cbar"]))
    fa = rc.excess(a64["alc"], a80["alc"], a80["abar"])
    live = np.asarray(a80["alc"], dtype=np.float64) > 0.
    ratio = float(np.max(a80["abar"][live] / np.asarray(a80["alc"], dtype=np.float64)[live])) if live.any() else 0.
    print("%s %s D=%d: alc_bar / ALC at most %.3g (largest ALC %.3g); float64 at %.3g of cov_bar and %.3g of alc_bar" % (
        *case, ratio, float(a80["alc"].max()), fc, fa))
    assert not a80["deg"].any() and not a64["deg"].any()
    if name in TIGHT:
        assert ratio < 0.05 and live.all()
        assert max(fc, fa) <= 2. / (D + 4)
    else:
        assert max(fc, fa) <= 0.01
    if name == "needle":
        assert not live.any() and not np.asarray(a80["C"]).any()


# ---- 5. greedy batches -----------------------------------------------------------------------------------------------------------------------
@CASES
def test_gaps_of_the_greedy_reference(case):
    name = case[0]
    if name == "needle":
        assert not np.asarray(rc.alc_reference(*case)["alc"]).any()       # every score an exact zero: nothing to pick, no gap to speak of
        return
    g = rc.batch_reference(*case)
    print("%s %s D=%d: picks %s, top-two gaps in bars %s" % (*case, g["picks"][0], np.array2string(g["gap"][0], precision=3)))
    if name in TIGHT:
        assert np.all(g["gap"] >= GAP)
    steps = rc.batch_steps(*case, tuple(int(i) for i in g["picks"][0]))
    # batch_steps on the reference's own picks is the reference (LAPACK's threading may move last bits: a tenth of the bars, which are a few ulps in the tight regimes)
    assert np.all(np.abs(steps["alc"] - g["alc"][0]) <= 0.1 * g["bar"][0]) and np.all(np.abs(steps["iv"] - g["iv"][0]) <= 0.1 * g["iv_bar"][0])


# ---- 2. paths: value and gradient ----------------------------------------------------------------------------------------------------------------
@CASES
def test_float64_paths_lie_inside_the_bars_on_their_own_fields(case):
    """value and gradient of three paths (130 features) from the fields of a float64 restated draw, float64 against long double on THE SAME
    update: the bars of regime_cases.path_truth hold float64 arithmetic itself, far inside"""
    import iterative_restate as ir
    r = rc.regime(*case)
    omega, phase = pw.features(rc.PATH_SEED, rc.PATH_STREAM, rc.PATH_F, case[2], r.kernel)
    W, eps = rc.path_normals()
    _, v, _ = pw.paths(r.X, r.t, r.Xs, rc.scales(r), r.kernel, rc.sigma2(r), r.nugget, omega, phase, W, eps)
    v80, vbar, g80, gbar = rc.path_truth(r, omega, phase, W, v)
    v64, _, g64, _ = rc.path_truth(r, omega, phase, W, v, np.float64)
    fv, fg = rc.excess(v64, v80, vbar), rc.excess(g64, g80, gbar)
    print("%s %s D=%d: float64 paths at %.3g (value) and %.3g (gradient) of their bars" % (*case, fv, fg))
    assert fv <= 0.1 and fg <= 0.1


# ---- 7. mixtures and joint draws -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", rc.MIX_WEIGHTS)
@pytest.mark.parametrize("kernel", rc.KERNELS)
def test_the_mixture_of_every_regime_is_fit_to_judge_a_kernel_with(kernel, wkind):
    a, bars, dis = rc.mixture_reference(kernel, wkind)
    th = rc.mixture_thetas(kernel)
    print("%s %s weights: float64 vs long double: %s; log sigma^2 spans %.3g, log nugget %.3g" % (
        kernel, wkind, ", ".join("%s %.3g" % kv for kv in dis.items()), np.ptp(th[:, -2]), np.ptp(th[:, -1])))
    assert max(dis.values()) <= rc.ILL and np.ptp(th[:, -2]) == 36. and np.ptp(th[:, -1]) > 36.                # e^36: sixteen orders of magnitude
    assert abs(a["weights"].sum() - 1.) < 1e-14 and np.all(a["weights"] > 0.)


@CASES
def test_which_regimes_need_a_rung_of_the_ladder(case):
    """recorded, and asserted where it is certain: with the nugget Sigma~ of the 37 queries factorises as it is in every regime (its
    smallest eigenvalue is at least eta); without it `long` and the regimes whose queries the design determines to rounding may not"""
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    cov = np.asarray(ref["fullcov"], dtype=np.float64)              # with the nugget on its diagonal
    with_n, without = rc.ladder_rung(cov - r.nugget * np.eye(rc.M), r.nugget), rc.ladder_rung(cov - r.nugget * np.eye(rc.M), 0.)
    ev = np.linalg.eigvalsh(cov)
    print("%s %s D=%d: Sigma~ eigenvalues %.3g .. %.3g; ladder rung with the nugget %d, without %d" % (*case, ev[0], ev[-1], with_n, without))
    assert with_n == 0
    if case[0] == "needle":
        s2 = rc.sigma2(r)
        assert np.array_equal(cov, (s2 + r.nugget) * np.eye(rc.M)) and without == 0


# ---- 6. the variance bound -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank", rc.VAR_RANKS)
@CASES
def test_restated_variance_bound_is_never_below_the_dense_variance(case, rank):
    """the restatement on its own pivots: the rank its cache reaches (K ~ sigma^2 I has no pivot order, K ~ sigma^2 1 1^T is of rank 1 and the
    factor runs out), and bound >= the long-double dense variance - bar; at rank N with a full cache the two agree to the bar"""
    import variance_bound_restate as vr
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    K, ks, _ = rc.bound_inputs(*case)
    ch, bar, cond, amp, own, first = rc.bound_cache(*case, rank)
    gap = vr.bound(ch.R, ks, rc.sigma2(r), r.nugget) - np.asarray(ref["var"], dtype=np.float64)
    print("%s %s D=%d rank %d: factor of rank %d, var_rank %d, cond(H) %.3g; the first %d columns determined (largest own error before %.3g, "
          "behind %.3g of the bar over %d evaluations of K); (bound - dense) / bar in [%.3g, %.3g]" % (
              *case, rank, ch.L.shape[1], ch.var_rank, cond, first, float(np.max(own[:first])) if first else 0.,
              float(np.max(own[first:])) if first < ch.var_rank else 0., rc.OWN_TRIALS + 1, gap.min() / bar, gap.max() / bar))
    assert ch.var_rank >= 1 and np.all(gap >= -bar)
    # what a device result can be held to column by column: the columns before the pivots of the first prefix fall towards tau (10 of 16 to
    # 121 of 121 in the cut caches, 18 of 32 in `long` at rank 32, every column elsewhere: printed above); behind them the restatement is up
    # to hundreds of bars from itself
    assert 1 <= first <= ch.var_rank, (first, ch.var_rank)
    if case[0] != "long" and ch.var_rank == ch.L.shape[1]:
        assert first == ch.var_rank                          # nothing cut, K not of rank 1: every column is determined
    assert first == ch.var_rank or float(np.max(own[first:])) > 1.
    if ch.var_rank == rc.N:
        assert np.all(np.abs(gap) <= bar)
