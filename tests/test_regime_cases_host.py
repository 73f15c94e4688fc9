"""The hyperparameter regimes of regime_cases.py are fit to judge a kernel with: no device here.  For every regime and kernel

  * cond(K + eta I) <= 1e7, so dimension_cases.amplification gives 1 and the project's bars apply unchanged;
  * the float64 restatement of every quantity test_gpu_regimes.py compares lies within 0.01 of that quantity's bar from the long-double
    one -- the bar is never about the reference (the Hessian's and cross-validation's bars are 100 x this disagreement by construction;
    for them the rule of their own files is asserted: the disagreement stays below 1e-8);
  * the share of entries of K whose long-double value lies below the smallest normal double is 0 except in `underflow` (SE only: the
    Matern's argument sqrt(5 r2) reaches 170 there, far from 708) and `needle`.

One pair misses the second point and is named in FLOAT64_EXCEPTIONS with its reason.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import dimension_cases as dc
import local_restate as lr
import regime_cases as rc
import vecchia_restate as vr

SHARE = 0.01
COND_LIMIT = 1e7

# big_sigma, full covariance: its entries between distant queries are of order 1 where the matrices they are the difference of are of
# order sigma^2 = 6.6e7, and BARS["fullcov"]'s absolute part does not grow with sigma^2: float64 arithmetic itself leaves 1e-15 sigma^2 =
# 6e-8 there, 0.016 of the bar (measured: SE 0.016, Matern 0.0016, product 0.0006).  The device is held to the full bar all the same;
# here the restatement must stay inside a tenth of it.
FLOAT64_EXCEPTIONS = {("big_sigma", "fullcov"): 0.1}


def _ids(c):
    return "%s-%s-D%d" % c


def _share(tag, a, b, gscale=1.):
    """|float64 - long double| over the bar of tag, taken in long double so that the difference itself is exact"""
    rtol, atol = dc.BARS[tag]
    return float(np.max(np.abs(np.asarray(a).astype(rc.LD) - b) / (atol * gscale + rtol * np.abs(b))))


@pytest.mark.parametrize("case", rc.cases(rc.DENSE_KERNELS), ids=_ids)
def test_dense_quantities(case):
    name, kernel, D = case
    a, b = rc.dense_reference(name, kernel, D, np.float64), rc.dense_reference(name, kernel, D)
    print("%s %s D=%d: cond %.3g" % (name, kernel, D, b["cond"]))
    assert b["cond"] <= COND_LIMIT and b["amp"] == 1.
    gscale = max(1., float(np.abs(a["grad"]).max()))
    for tag in dc.BARS:
        share = _share(tag, a[tag], b[tag], gscale if tag == "grad" else 1.)
        print("  %-8s float64 restatement at %.3g of the bar" % (tag, share))
        assert share <= FLOAT64_EXCEPTIONS.get((name, tag), SHARE), (case, tag, share)
    if name == "needle":
        want = rc.needle_closed_form(rc.regime(name, kernel, D))
        for tag in dc.BARS:
            assert _share(tag, np.asarray(b[tag], dtype=np.float64), want[tag]) <= SHARE, tag


@pytest.mark.parametrize("case", rc.cases(), ids=_ids)
def test_share_of_entries_below_the_smallest_normal_double(case):
    name, kernel, D = case
    r = rc.regime(name, kernel, D)
    U, Us = rc.staged(r, r.X), rc.staged(r, r.Xs)
    assert np.array_equal(rc.scales(r), rc.scales_libm(r))      # NumPy's exp and the C library's give the same scales here
    sub = zero = total = 0
    for A in (U, Us):
        k = rc.sigma2(r) * rc.entries(A, U, kernel)[0]
        sub, zero, total = sub + int(np.sum(k < rc.TINY)), zero + int(np.sum(k < rc.LD(rc.STEP) / 2)), total + k.size
    print("%s %s D=%d: %.4f of the entries of K and K* below the smallest normal double, %.4f below half a subnormal step" % (
        name, kernel, D, sub / total, zero / total))
    if name == "needle":
        assert zero == total - r.X.shape[0]                    # everything but K's diagonal
    elif name == "underflow" and kernel == "SquaredExponential":
        assert 0 < sub - zero and 0 < zero                     # subnormal results and results that round to 0
    else:
        assert sub == 0
    if name == "twin":
        r2 = np.sum((U[-1] - U[0]) ** 2)
        assert 1e-18 < r2 < 1e-16


@pytest.mark.parametrize("fit", [False, True], ids=["fixed", "fit"])
@pytest.mark.parametrize("case", rc.cases(), ids=_ids)
def test_hessian_cases_are_not_ill_conditioned(case, fit):
    h = rc.hessian_reference(*case, fit)
    print("%s %s D=%d %s: float64 vs long double %.3g of max|H| = %.4g%s" % (*case, "fit" if fit else "fixed", h["dis"], h["scale"],
                                                                            " (below n 2^-52: the floor is the bar)" if h["floored"] else ""))
    assert h["dis"] <= rc.ILL and np.all(np.isfinite(h["H"]))


@pytest.mark.parametrize("k", [None, rc.CV_FOLDS], ids=["loo", "k5"])
@pytest.mark.parametrize("case", rc.cases(), ids=_ids)
def test_cross_validation_cases_are_not_ill_conditioned(case, k):
    a, b = rc.cv_reference(*case, k)
    for q, (dis, scale) in rc.cv_disagreement(rc.regime(*case), a, b).items():
        print("%s %s D=%d %s: float64 vs long double, %s %.3g of %.4g" % (*case, "loo" if k is None else "k=5", q, dis, scale))
        assert dis <= rc.ILL, (case, q, dis)


@pytest.mark.parametrize("case", rc.cases(), ids=_ids)
def test_local_and_vecchia_quantities(case):
    """k = 30 on the restatement's own lists: every local matrix factorises, cond <= 1e7, float64 within 0.01 of the bars.  (In `long` the
    float64 restatement of single Vecchia terms takes 0.035 of the per-term bar of test_gpu_vecchia.py; their sum, which is what is compared on
    the device, 2e-4.)"""
    name, kernel, D = case
    r = rc.regime(name, kernel, D)
    s = rc.scales(r)
    nbr = lr.neighbours(r.X, r.Xs, s, rc.K_LOCAL)[0]
    m64, v64, ok64, cond = rc.local_reference(r, nbr, np.float64)
    m80, v80, ok80, _ = rc.local_reference(r, nbr)
    assert ok64.all() and ok80.all() and cond.max() <= COND_LIMIT
    sm, sv = _share("mean", m64, m80), _share("var", v64, v80)
    vn = vr.ordered_neighbours(r.X, s, rc.K_LOCAL)
    t64, g64, o64, vcond = rc.vecchia_reference(r, vn, np.float64)
    t80, g80, o80, _ = rc.vecchia_reference(r, vn)
    assert o64.all() and o80.all() and vcond.max() <= COND_LIMIT
    st = _share("logpost", t64, t80)                  # printed only: the device test compares the value and the gradient, not single terms
    sl = _share("logpost", t64.sum(), t80.sum())
    sg = _share("grad", g64.sum(axis=0), g80.sum(axis=0), max(1., float(np.abs(g64.sum(axis=0)).max())))
    print("%s %s D=%d: local cond %.3g mean %.3g var %.3g | Vecchia cond %.3g terms %.3g value %.3g gradient %.3g of their bars" % (
        name, kernel, D, cond.max(), sm, sv, vcond.max(), st, sl, sg))
    assert max(sm, sv, sl, sg) <= SHARE


@pytest.mark.parametrize("case", rc.cases(), ids=_ids)
def test_restated_pcg_converges_and_its_mean_is_the_dense_one(case):
    """the convergence condition of the iterative paths: iterative_restate's solver, at the rank, tolerance and limit the device test uses,
    converges inside test_iterative_host.py's cap in every regime, and its mean lies within 0.01 of the bar from the long-double dense one"""
    import iterative_restate as ir
    r, ref = rc.regime(*case), rc.dense_reference(*case)
    mean, _, sa, _ = ir.predict(r.X, r.t, r.Xs, rc.scales(r), r.kernel, rc.sigma2(r), r.nugget, rc.ITER_RANK, rc.ITER_RTOL, rc.ITER_MAX, want_var=False)
    share = float(np.max(np.abs(mean.astype(rc.LD) - ref["mean"]) / rc.exact_mean_bar(ref, r, sa.x[:, 0])))
    print("%s %s D=%d: %d iterations, residual %.3g, mean at %.3g of its bar" % (*case, sa.iterations[0], sa.residual[0], share))
    assert sa.converged.all() and sa.iterations[0] <= rc.ITER_CAP and share <= SHARE
