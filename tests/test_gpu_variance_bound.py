"""The variance bound on the MI355X (mogp_emulator_amd.IterativeGP variance_bound / variance_cache / variance_gap / predict(unc="bound");
csrc/kernels_iter.hip kvar_kernel and tri_right_kernel, csrc/engine_iter.hip) against the NumPy restatement (variance_bound_restate.py) on the
device's own pivots, the dense GaussianProcessGPU.predict and the exact predict(unc=True).

Shapes: designs of three and five row tiles with a partial last one, and 1000 points once; 37 and 65 queries (a partial and a second query
tile); input dimensions 1, 3, 17 and 80; the four kernels; ranks on both sides of a block of 16 and of a chunk of VAR_CHUNK columns, rank N, and
the designs on a line where the cache stops below the preconditioner's rank.  The two-sided comparison with the restatement is what catches a
dropped column or tile: a sum of squares that is too small still bounds the variance.

The columns of the cache are compared one by one wherever the restatement determines them to the bar (everywhere unless the first prefix
is cut by tau; there the last column kept differs by 4.3 bars between two float64 evaluations of the restatement itself, by 2.99 on the
device: test_variance_bound_host.reference_own_error); R^T A R = I and the bound hold every column.

The bar is that of test_variance_bound_host.py: dc.BARS of the quantity, amplified by cond(H) of the restatement's H = Q^T A Q.  Hyperparameters
come from a GaussianProcessGPU fitted on the first 64 rows.  Measured figures are printed as fractions of their bars; DESIGN.md section 3
"Variance bound" records them."""
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import iterative_restate as ir
import test_iterative_host as th
import test_variance_bound_host as vh
import variance_bound_restate as vr
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu

SUB = 64
CHUNK = M.IterativeGP.VAR_CHUNK
CASES = ([(130, 1, "SquaredExponential", 32), (130, 3, "Matern52", 130), (130, 17, "SquaredExponential", 130), (130, 80, "Matern52", 32),
          (300, 1, "UniformSqExp", 64), (300, 3, "UniformMat52", 300), (1000, 5, "SquaredExponential", 256)]
         + [(300, 3, k, 64) for k in th.FOUR])
FULL = [(130, 3, "Matern52", 130), (130, 17, "SquaredExponential", 130), (300, 3, "UniformMat52", 300)]


def _gp(X, t, kernel, theta):
    gp = M.GaussianProcessGPU(X, t, kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=dc.n_corr(kernel, X.shape[1]), nugget_type="fixed"))
    gp.fit(theta)
    return gp


def _iter(c, kernel, p, **kw):
    n = c.X.shape[0]
    gp = _gp(c.X[:min(SUB, n)], c.T[0, :min(SUB, n)], kernel, c.thetas[0])
    return M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER, **kw)


@functools.lru_cache(maxsize=None)
def _dense(n, D, kernel):
    """(K without the nugget, A, cross covariances of the 65 queries (n, 65)) of one shape, computed once and never changed"""
    c, (s,) = th.setup(n, D, kernel, m=vh.M_Q)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    A = K + dc.NUGGET * np.eye(n)
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    for a in (K, A, ks):
        a.setflags(write=False)
    return K, A, ks


@pytest.mark.parametrize("n,D,kernel,p", CASES, ids=lambda v: str(v))
def test_cache_and_bound_against_the_restatement_and_the_exact_variances(n, D, kernel, p):
    c, (s,) = th.setup(n, D, kernel, m=vh.M_Q)
    c37, _ = th.setup(n, D, kernel, m=dc.M_TEST[0])           # (the same design; a partial query tile alone)
    K, A, ks = _dense(n, D, kernel)
    ig = _iter(c, kernel, p)
    L, piv = ig.preconditioner()
    R, vrank = ig.variance_cache()
    R2, vrank2 = ig.variance_cache()
    reached = len(piv)
    assert R.shape == (n, vrank) and vrank2 == vrank and np.array_equal(R, R2) and 1 <= vrank <= reached <= p
    ch = vr.cache(K, dc.NUGGET, reached, pivots=piv)
    bar, cond, amp = vh.slack(ch.H)
    early = (n, D, kernel, p) in vh.EARLY_STOP
    if early:
        assert vrank < reached and ch.var_rank < reached      # L's last columns are rounding noise: both prefixes stop before them
    else:
        assert vrank == ch.var_rank == reached
    rr = min(vrank, ch.var_rank)
    assert rr >= vrank - 1 and rr >= ch.var_rank - 1, (vrank, ch.var_rank)
    # ---- the cache: column by column wherever the restatement itself determines the column to the bar (every column unless the first
    # prefix is cut by tau: test_variance_bound_host.py shows the restatement 4.3 bars from itself in the last column it keeps at
    # (300, 1, UniformSqExp, 64) when K changes by one ulp); R^T A R = I and the two-sided bound below hold the other columns
    own = vh.reference_own_error(c, s, kernel, ch, amp)[:rr]
    cols = vh.column_excess(R[:, :rr], ch.R[:, :rr], amp)
    assert early or np.all(own <= 1.)
    e_R, e_R_all = float(np.max(cols[own <= 1.])), float(np.max(cols))
    e_I = dc.excess("fullcov", R.T @ A @ R, np.eye(vrank), amp)
    # ---- the bound, two-sided against the restatement, on both query counts
    got = ig.variance_bound(c.Xs, rank=rr)
    assert got.shape == (vh.M_Q,) and np.all(np.isfinite(got)) and np.array_equal(got, ig.variance_bound(c.Xs, rank=rr))
    e_b = dc.excess("var", got, vr.bound(ch.R, ks, SIGMA2, dc.NUGGET, rank=rr), amp)
    k37 = ir.covariance(c.X, c37.Xs, s, kernel, SIGMA2)
    got37 = ig.variance_bound(c37.Xs, rank=rr)
    e_b37 = dc.excess("var", got37, vr.bound(ch.R, k37, SIGMA2, dc.NUGGET, rank=rr), amp)
    # ---- never over-confident: the dense predict at the same theta, and the exact iterative variance
    full = ig.variance_bound(c.Xs)
    dense = _gp(c.X, c.T[0], kernel, c.thetas[0]).predict(c.Xs, deriv=False).unc
    exact = ig.predict(c37.Xs, unc=True)
    gap_d, gap_e = full - dense, ig.variance_bound(c37.Xs) - exact.unc
    # exact algebra for an inexact solve: |k*^T (x - A^-1 k*)| <= |A^-1 k*| |k* - A x|, as test_gpu_iterative.py allows the exact variance
    solver = np.linalg.norm(np.linalg.solve(A, k37), axis=0) * exact.var_residual * np.linalg.norm(k37, axis=0)
    print("n %d D %d %s p %d: rank reached %d, var_rank %d (restatement %d), cond(H) %.3g; R at %.3g of its bar on the %d of %d columns the restatement "
          "determines (%.3g on all; the restatement's own error %.3g), R^T A R - I at %.3g; bound against the "
          "restatement at %.3g (65 queries) and %.3g (37) of its bar; (bound - dense) / sigma^2 mean %.3g max %.3g min %.3g; bound - exact min %.3g "
          "(slack %.3g)" % (n, D, kernel, p, reached, vrank, ch.var_rank, cond, e_R, int(np.count_nonzero(own <= 1.)), rr, e_R_all, float(np.max(own)),
                          e_I, e_b, e_b37, gap_d.mean() / SIGMA2, gap_d.max() / SIGMA2,
                          gap_d.min() / SIGMA2, gap_e.min(), bar))
    ig.close()
    assert e_R <= 1. and e_I <= 1.
    assert e_b <= 1. and e_b37 <= 1.
    assert np.all(full <= got)                                 # (more columns never give more)
    assert exact.var_converged.all()
    assert np.all(gap_d >= -bar) and np.all(gap_e >= -(bar + solver))
    if (n, D, kernel, p) in FULL:
        assert np.max(np.abs(gap_d)) <= bar and np.all(np.abs(gap_e) <= bar + solver)      # the exact variance at rank N


def test_ranks_on_both_sides_of_a_block_and_of_a_chunk():
    n, D, kernel = 300, 3, "SquaredExponential"
    ranks = [min(r, n) for r in (16, 17, CHUNK - 1, CHUNK, CHUNK + 1)]
    p = 2 * CHUNK + 1
    c, (s,) = th.setup(n, D, kernel, m=vh.M_Q)
    K, A, ks = _dense(n, D, kernel)
    ig = _iter(c, kernel, p)
    piv = ig.preconditioner()[1]
    R, vrank = ig.variance_cache()
    assert vrank == p
    ch = vr.cache(K, dc.NUGGET, p, pivots=piv)
    bar, cond, amp = vh.slack(ch.H)
    prof = vr.profile(ch.R, ks, SIGMA2, dc.NUGGET)
    last = None
    for r in [1] + ranks + [2 * CHUNK, p]:
        got = ig.variance_bound(c.Xs, rank=r)
        e = dc.excess("var", got, prof[r], amp)
        if last is not None:
            assert np.all(got <= last), r                      # non-increasing in the rank, exactly
        last = got
        own = e
        if r in ranks:                                         # the leading columns are the cache of a handle of that rank
            small = _iter(c, kernel, r)
            own = dc.excess("var", small.variance_bound(c.Xs), got, amp)
            assert small.variance_cache()[1] == r
            small.close()
        print("rank %d: bound at %.3g of its bar against the restatement, at %.3g against a handle of that precond_rank" % (r, e, own))
        assert e <= 1. and own <= 1.
    assert np.array_equal(last, ig.variance_bound(c.Xs))      # rank=None: all of the cache
    with pytest.raises(RuntimeError, match="variance_bound: precond_rank must be between 0 and"):
        ig._native.variance_bound(*ig._hyper[0][:4], n + 1, True, c.Xs)
    with pytest.raises(RuntimeError, match="variance_bound: the variance bound is built from the preconditioner's factor"):
        ig._native.variance_bound(*ig._hyper[0][:4], 0, True, c.Xs)
    with pytest.raises(RuntimeError, match="variance_bound: rank must be between 1 and the rank the preconditioner reached, %d" % p):
        ig._native.variance_bound(*ig._hyper[0][:4], p, True, c.Xs, var_rank=p + 1)
    ig.close()


def test_a_rank_beyond_the_rank_reached_is_refused_by_name():
    n, D, kernel, p = vh.EARLY_STOP[0]
    c, (s,) = th.setup(n, D, kernel, m=dc.M_TEST[0])
    ig = _iter(c, kernel, p)
    reached = len(ig.preconditioner()[1])
    R, vrank = ig.variance_cache()
    assert vrank < reached < p and np.all(np.isfinite(R))
    with pytest.raises(RuntimeError, match="variance_bound: rank must be between 1 and the rank the preconditioner reached, %d" % reached):
        ig.variance_bound(c.Xs, rank=reached + 1)
    a, b = ig.variance_bound(c.Xs, rank=reached), ig.variance_bound(c.Xs)       # the columns the cache does not have add nothing
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    ig.close()


def test_bound_depends_on_its_query_alone():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, (s,) = th.setup(n, D, kernel, m=vh.M_Q)
    ig = _iter(c, kernel, p)
    first = ig.variance_bound(c.Xs)
    assert np.array_equal(ig.variance_bound(c.Xs), first)
    for j in (0, 5, 36, 63, 64):
        assert ig.variance_bound(c.Xs[j:j + 1])[0] == first[j], j
    for mp in (1, 7, 64):
        assert np.array_equal(ig.variance_bound(c.Xs, max_points=mp), first), mp
    assert np.array_equal(ig.variance_bound(c.Xs[::-1].copy())[::-1], first)
    ig.close()


def test_predict_with_the_bound():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, (s,) = th.setup(n, D, kernel, m=vh.M_Q)
    ig = _iter(c, kernel, p)
    bare = ig.predict(c.Xs)
    pr = ig.predict(c.Xs, unc="bound")
    want = ig.variance_bound(c.Xs)
    assert np.array_equal(pr.mean, bare.mean) and np.array_equal(pr.unc, want)
    assert pr.var_converged is None and pr.var_residual is None and pr.unc_kind == "bound" and pr.var_rank == p
    assert bare.unc is None and bare.unc_kind is None and bare.var_rank is None
    for mp in (1, 7):
        q = ig.predict(c.Xs, unc="bound", max_points=mp)
        assert np.array_equal(q.mean, pr.mean) and np.array_equal(q.unc, pr.unc)
    with pytest.raises(ValueError, match='unc must be False, True or "bound"'):
        ig.predict(c.Xs, unc="Bound")
    # without the nugget: lower by it, to the three roundings of the two differences
    nn = ig.predict(c.Xs, unc="bound", include_nugget=False)
    assert np.array_equal(nn.mean, pr.mean) and np.array_equal(nn.unc, ig.variance_bound(c.Xs, include_nugget=False))
    live = nn.unc > 0.
    assert live.any() and np.all(np.abs((pr.unc - nn.unc)[live] - dc.NUGGET) <= 2. * 2. ** -52 * (SIGMA2 + dc.NUGGET))
    assert np.all(pr.unc[~live] <= dc.NUGGET + 2. * 2. ** -52 * (SIGMA2 + dc.NUGGET))
    # the user's own check of the gap
    few = c.Xs[:5]
    gap = ig.variance_gap(few)
    exact = ig.predict(few, unc=True)
    assert exact.unc_kind == "exact" and exact.var_rank is None
    assert gap.shape == (5,) and np.array_equal(gap, ig.variance_bound(few) - exact.unc)
    ig.close()


def test_multi_output_rows_are_the_single_emulator_calls():
    n, D, kernel, p, E, nq = th.MULTI
    c, scales = th.setup(n, D, kernel, E=E)
    mo = M.MultiOutputGP_GPU(c.X[:SUB], c.T[:, :SUB], kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=c.nc, nugget_type="fixed"))
    mo.fit(c.thetas)
    ig = M.IterativeGP(mo, c.X, c.T, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    pr = ig.predict(c.Xs[:nq], unc="bound")
    assert pr.mean.shape == pr.unc.shape == (E, nq) and pr.var_rank.shape == (E,) and pr.var_converged is None and pr.unc_kind == "bound"
    for e in (2, 0, 1):                                        # (out of order: the cache of another emulator is the one held)
        ge = _gp(c.X[:SUB], c.T[e, :SUB], kernel, c.thetas[e])
        one = M.IterativeGP(ge, c.X, c.T[e], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        q = one.predict(c.Xs[:nq], unc="bound")
        assert np.array_equal(q.mean, pr.mean[e]) and np.array_equal(q.unc, pr.unc[e]) and q.var_rank == pr.var_rank[e]
        assert np.array_equal(ig.variance_bound(c.Xs[:nq], emulator=e), pr.unc[e])
        assert np.array_equal(one.variance_cache()[0], ig.variance_cache(emulator=e)[0])
        one.close()
    assert not np.array_equal(pr.unc[0], pr.unc[1]) and not np.array_equal(pr.unc[1], pr.unc[2])
    ig.close()


def test_vecchia_predict_exact_passes_the_bound_through():
    n, D, kernel, p = 300, 3, "SquaredExponential", 64
    c, (s,) = th.setup(n, D, kernel)
    kw = dict(precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, order=np.arange(n))
    got = vg.predict_exact(c.Xs, theta=c.thetas[0], unc="bound", **kw)
    view = vg.exact_view(c.thetas[0], **kw)
    assert got.unc_kind == "bound" and got.var_rank == p and got.var_converged is None
    assert np.array_equal(got.unc, view.variance_bound(c.Xs)) and np.array_equal(got.mean, vg.predict_exact(c.Xs, theta=c.thetas[0], **kw).mean)
    vg.close()
    ig = _iter(c, kernel, p)                                   # the caller's order kept: the same data on the handle, hence the same bits
    assert np.array_equal(ig.variance_bound(c.Xs), got.unc)
    ig.close()
