"""The large-design paths past one block and one problem per workgroup, on the MI355X: LocalGP and VecchiaGP with more problems than the
persistent grid has workgroups (every workgroup takes a second problem and some a third: csrc/kernels_local.hip local_gp_kernel and
vecchia_ll_kernel), the second pass of the Vecchia sum (launch_vecchia_reduce), and IterativeGP at N = 1030 and N = 4100: a second, partial
block of 1024 rows in the dots (cg_dot_kernel, cg_scalars_kernel) and in the pivot search (pchol_argmax1/2_kernel), a second, partial segment
of 4096 rows in the preconditioner's L^T R (ltv_kernel, sum_parts_kernel; csrc/kernels_iter.hip).  Every other GPU test of these features
stays below those sizes: there the second stage of every reduction adds one summand and no workgroup takes a second problem.

The grid is not written down here: it is LOCAL_GRID_PER_CU = 4 workgroups per compute unit of the device the tests run on (the rule of
csrc/predict_plan.h, pinned on the host by tests/c/local_plan_check.cpp), and a count that cannot be read fails the test.

Two kinds of check.  Bits: the one big call against the same work sent in launches of at most `grid` problems, the one-problem-per-workgroup
path that test_gpu_local.py and test_gpu_vecchia.py verify.  Values: against the NumPy restatements at the bars of the tests of each feature,
whose checks are run here on the larger shapes as they stand.  large_design_cases.py holds shapes and inputs; test_large_design_host.py shows
on the CPU that the references alone meet every condition used here.  Measured figures are printed as fractions of their bars; DESIGN.md
section 3 "Large designs past one block" records them."""
import math

import numpy as np
import pytest

import mogp_emulator_amd as M

import dimension_cases as dc
import iterative_restate as ir
import large_design_cases as ld
import local_cases as lc
import local_restate as lr
import test_gpu_exact_lik as te
import test_gpu_iterative as tg
import test_gpu_local as tl
import test_gpu_variance_bound as tb
import test_gpu_vecchia as tv
import test_iterative_host as th
import vecchia_cases as vc
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu


def _grid():
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return ld.grid_of(cus)


# ---- A. LocalGP: several queries per workgroup ----------------------------------------------------------------------------------------------
def _local(kernel, grid):
    c, s = ld.local_setup(kernel, grid)
    gp = tl._gp(c.X[:tl.SUB], c.T[0, :tl.SUB], kernel, c.thetas[0])
    return c, s, M.LocalGP(gp, c.X, c.T[0], n_neighbours=ld.LOCAL["k"])


@pytest.mark.parametrize("kernel", ld.LOCAL_KERNELS)
def test_local_one_call_is_the_one_problem_per_workgroup_passes_bit_for_bit(kernel):
    grid = _grid()
    m = ld.local_m(grid)
    c, s, lg = _local(kernel, grid)
    big = lg.predict(c.Xs, return_neighbours=True)
    passes = lg.predict(c.Xs, return_neighbours=True, max_points=grid)
    assert big.mean.shape == (m,) and big.ok.all() and big.n_failed == 0
    assert tl._bits(big) == tl._bits(passes)
    for j in ld.local_singles(grid):
        one = lg.predict(c.Xs[j:j + 1], return_neighbours=True)
        assert (one.mean[0].tobytes(), one.unc[0].tobytes(), one.radius[0].tobytes(), bool(one.ok[0])) == (
            big.mean[j].tobytes(), big.unc[j].tobytes(), big.radius[j].tobytes(), True), j
        assert np.array_equal(one.neighbours[0], big.neighbours[j]), j
    lg.close()
    print("grid %d, %d queries, %s: one call, passes of %d and single queries agree bit for bit" % (grid, m, kernel, grid))


@pytest.mark.parametrize("kernel", ld.LOCAL_KERNELS)
def test_local_neighbours_exactly_and_values_within_the_bars_on_every_row(kernel):
    grid = _grid()
    c, s, lg = _local(kernel, grid)
    ref = ld.local_reference(kernel, grid)
    p = lg.predict(c.Xs, return_neighbours=True)
    lg.close()
    assert p.ok.all() and np.array_equal(p.neighbours, ref["nbr"])
    assert np.array_equal(p.radius.view(np.int64), ref["radius"].view(np.int64))
    em, ev = lc.excess_rows("mean", p.mean, ref["mean"], ref["cond"]), lc.excess_rows("var", p.unc, ref["var"], ref["cond"])
    print("grid %d, %d queries, %s: mean at %.3g of its bar, variance at %.3g (cond at most %.3g)" % (grid, p.mean.shape[0], kernel, em, ev, ref["cond"].max()))
    assert em <= 1. and ev <= 1.


def test_local_failure_stays_in_its_problem():
    """The first `grid` queries meet exactly singular matrices (every far point twice, nugget 0), and the workgroup that refused query j goes
    on to the clean query j + grid: the status word, the pack of the factorisation and the scratch tile are that workgroup's own."""
    grid = _grid()
    X, t, Q, s, n_far = ld.local_failure(grid)
    kernel, k = ld.LOCAL_FAIL_KERNEL, ld.LOCAL["k"]
    c, _ = ld.local_setup(kernel, grid)
    gp = tl._gp(c.X[:tl.SUB], c.T[0, :tl.SUB], kernel, c.thetas[0], nugget=0.)
    lg = M.LocalGP(gp, X, t, n_neighbours=k)
    big = lg.predict(Q, return_neighbours=True)
    passes = lg.predict(Q, return_neighbours=True, max_points=grid)
    lg.close()
    assert tl._bits(big) == tl._bits(passes)                                             # NaN pattern and ok included
    assert np.array_equal(~big.ok, np.isnan(big.mean)) and np.array_equal(~big.ok, np.isnan(big.unc)) and big.n_failed == int(np.sum(~big.ok))
    assert np.all(big.neighbours[:grid] >= ld.LOCAL["N"]) and np.all(big.neighbours[grid:] < ld.LOCAL["N"])
    refused = ~passes.ok[:grid]
    print("grid %d: %d of %d far-region queries refused, %d of %d clean ones" % (grid, refused.sum(), grid, np.sum(~big.ok[grid:]), Q.shape[0] - grid))
    assert np.any(refused & big.ok[grid:2 * grid])                                       # some j: not ok[j] and ok[j + grid]
    assert big.ok[grid:].all()                                                           # (the restatement accepts every clean query with room)
    mean, var, ok, cond = lr.predict(X, t, Q[grid:], s, kernel, SIGMA2, 0., big.neighbours[grid:])
    em, ev = lc.excess_rows("mean", big.mean[grid:], mean, cond), lc.excess_rows("var", big.unc[grid:], var, cond)
    print("    clean queries behind them: mean at %.3g of its bar, variance at %.3g (cond at most %.3g)" % (em, ev, cond.max()))
    assert ok.all() and em <= 1. and ev <= 1.


# ---- B. Vecchia: several points per workgroup and the second pass of the sum ------------------------------------------------------------------
def _ll_bits(ll):
    return (np.float64(ll.value).tobytes(), ll.grad.tobytes(), ll.terms.tobytes(), ll.ok.tobytes())


@pytest.mark.parametrize("kernel,fit", ld.VECCHIA_CASES)
def test_vecchia_bits_terms_and_the_sum(kernel, fit):
    grid = _grid()
    N, D, k = ld.vecchia_n(grid), ld.VECCHIA["D"], ld.VECCHIA["k"]
    c, theta, order, vg = tv._vecchia(N, D, k, kernel, fit, "random")
    ref = ld.vecchia_reference(kernel, fit, grid)
    vg.set_neighbours(theta=theta)
    assert np.array_equal(vc.to_positions(vg.neighbours, order), ref["nbr"])
    ll = vg.loglik(theta, grad=True, return_terms=True)
    for mp in ld.vecchia_launches(grid):
        assert _ll_bits(vg.loglik(theta, grad=True, return_terms=True, max_points=mp)) == _ll_bits(ll), mp
    vg.close()
    assert ll.ok.all() and ll.n_failed == 0 and ll.terms.shape == (N,) and ll.grad.shape == (len(theta),)
    # the terms, row by row
    et = vc.excess_rows("logpost", ll.terms[order], ref["terms"], ref["cond"])
    amp = max(1., float(ref["cond"].max()) * 1e-7)
    # the sum: any order of N float64 additions lies within (N - 1) 2^-53 sum |terms| of the exact sum of the device's own terms
    bound = (N - 1) * 2. ** -53 * float(np.sum(np.abs(ll.terms)))
    es = abs(ll.value - math.fsum(ll.terms)) / bound
    ev = dc.excess("logpost", np.array([ll.value]), np.array([ref["terms"].sum()]), amp)
    eg = dc.excess("grad", ll.grad, ref["grad"].sum(axis=0), amp, max(1., float(np.max(np.abs(ll.grad)))))
    print("grid %d N %d %s nugget %s: terms at %.3g of their bar, value at %.3g of the sum's bound and %.3g of its bar, gradient at %.3g "
          "(cond at most %.3g)" % (grid, N, kernel, "fit" if fit else "fixed", et, es, ev, eg, ref["cond"].max()))
    assert amp == 1.
    assert et <= 1. and es <= 1. and ev <= 1. and eg <= 1.


def test_vecchia_failure_stays_in_its_point():
    grid = _grid()
    N, k, kernel = ld.vecchia_n(grid), ld.VECCHIA["k"], ld.VECCHIA_FAIL_KERNEL
    X, t, theta, s, sigma2, clean = ld.vecchia_failure(grid)
    ref = ld.vecchia_failure_reference(grid)
    vg = M.VecchiaGP(X, t, kernel=kernel, n_neighbours=k, nugget=0., order=np.arange(N))
    vg.set_neighbours(theta=theta)
    nbr = vg.neighbours
    ll = vg.loglik(theta, grad=True, return_terms=True)
    small = vg.loglik(theta, grad=True, return_terms=True, max_points=512)
    vg.close()
    assert ll.terms.tobytes() == small.terms.tobytes() and ll.ok.tobytes() == small.ok.tobytes()
    assert np.array_equal(~ll.ok, np.isnan(ll.terms)) and ll.n_failed == int(np.sum(~ll.ok)) and ll.value == -np.inf
    assert np.any(~ll.ok[:N - grid] & ll.ok[grid:])                                      # some j: not ok[j] and ok[j + grid]
    rows = ref["rows"]
    assert np.all(clean[np.maximum(nbr[rows], 0)])                                       # no clean list holds a far point
    assert np.array_equal(nbr[rows], ref["nbr"][rows])
    assert ll.ok[rows].all() and ref["ok"][rows].all()
    et = vc.excess_rows("logpost", ll.terms[rows], ref["terms"][rows], ref["cond"][rows])
    print("grid %d N %d: %d points refused, all of them in the far region; clean terms at %.3g of their bar (cond at most %.3g)"
          % (grid, N, ll.n_failed, et, ref["cond"][rows].max()))
    assert et <= 1.


# ---- C. IterativeGP: N = 1030 and N = 4100 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,kernel,p", ld.ITER_SOLVE_SHAPES, ids=lambda v: str(v))
def test_solve_converges_and_reports_its_true_residual(n, D, kernel, p):
    tg.test_solve_converges_and_reports_its_true_residual(n, D, kernel, p)


@pytest.mark.parametrize("n,D,kernel,p", ld.ITER_SOLVE_SHAPES, ids=lambda v: str(v))
def test_reported_residual_stays_within_the_drift_bound(n, D, kernel, p):
    tg.test_reported_residual_stays_within_the_drift_bound(n, D, kernel, p)


def test_a_column_that_lives_in_the_second_dot_block():
    """b is zero on the rows of the first block of 1024: were the second block's partial sum dropped, |b|^2 would be 0 and the column would
    freeze at iteration 0 with x = 0.  (Six nonzero entries make |x| = 10^4 |b|: 2^-52 | |A| |x| | = 2.8e-10 |b|, so the residual recomputed
    from x lies above rtol for any float64 solver -- the restatement reports 1.5e-10, a dense solve 2.1e-10 -- and the drift bound of the
    smooth right-hand sides does not apply to this column; what is reported must still be the true residual of x.)"""
    n, D, kernel, p = ld.ITER_TAIL
    c, s, ig = tg._iter(n, D, kernel, p)
    A, A80, cond, amp = tg._dense(n, D, kernel)
    B = ld.tail_column(n)
    sv = ig.solve(B)
    both = ig.solve(np.column_stack([c.T[0], B[:, 0]]))
    ig.close()
    host = tg._host_residual(A80, B, sv.x)
    slack = tg._residual_slack(A, B, sv.x, D, host)
    print("n %d %s p %d: the tail column took %d iterations, residual %.3g (host %.3g): their distance at %.3g of its bar"
          % (n, kernel, p, sv.iterations[0], sv.residual[0], host[0], abs(sv.residual[0] - host[0]) / slack[0]))
    assert sv.converged.all() and 1 <= sv.iterations[0] <= MAX_ITER and sv.x.any()
    assert np.all(np.abs(sv.residual - host) <= slack)
    assert host[0] <= RTOL + slack[0]                          # x solves the system: the recurrence's rtol and the roundings of A x (x = 0 gives 1)
    assert np.array_equal(both.x[:, 1], sv.x[:, 0]) and both.iterations[1] == sv.iterations[0]


def _check_pivots_are_maximisers(X, s, kernel, L, piv, what):
    K = ir.covariance(X, X, s, kernel, SIGMA2)
    want, piv_r, _ = ir.pivoted_cholesky(K, len(piv), pivots=piv)
    assert len(piv_r) == len(piv)
    d = ld.remaining_diagonals(K, want, piv)
    rtol, atol = dc.BARS["fullcov"]
    _, amp = dc.amplification(K[np.ix_(piv, piv)])
    bar = amp * (atol + rtol * SIGMA2)
    short = d.max(axis=1) - d[np.arange(len(piv)), piv]
    print("%s: the device's pivots miss the restatement's largest remaining diagonal by at most %.3g of the bar (amplification %.3g); L at %.3g"
          % (what, short.max() / bar, amp, dc.excess("fullcov", L, want, amp)))
    assert np.all(short <= bar) and dc.excess("fullcov", L, want, amp) <= 1.


def test_argmax_across_blocks():
    n, D, kernel, p = ld.ITER_OUTLIER
    c, s = ld.iter_setup(n, D, kernel)
    X = ld.outlier_design(c.X)
    gp = tg._gp(c.X[:tg.SUB], c.T[0, :tg.SUB], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    L, piv = ig.preconditioner()
    ig.close()
    assert len(piv) == p and len(set(piv.tolist())) == p
    assert piv[0] == 0                                        # the all-equal diagonal: a tie over both blocks goes to the lowest index
    assert piv[1] == ld.OUTLIER_ROW                           # the largest remaining diagonal lies in the second block
    _check_pivots_are_maximisers(X, s, kernel, L, piv, "n %d %s p %d, row %d moved out" % (n, kernel, p, ld.OUTLIER_ROW))


@pytest.mark.parametrize("n,D,kernel,p", ld.ITER_SOLVE_SHAPES, ids=lambda v: str(v))
def test_preconditioner_against_the_restatement_on_the_devices_pivots(n, D, kernel, p):
    tg.test_preconditioner_against_the_restatement_on_the_devices_pivots(n, D, kernel, p)
    c, s, ig = tg._iter(n, D, kernel, p)
    L, piv = ig.preconditioner()
    ig.close()
    _check_pivots_are_maximisers(c.X, s, kernel, L, piv, "n %d %s p %d" % (n, kernel, p))


def test_preconditioner_apply_across_segments():
    """w = P^-1 z of the likelihood's probe panel at N = 4100: L^T z is summed over two segments of rows.  With g1 = 0 and g2 zero on the
    first 4096 rows z lives in the second segment alone: dropping it gives exactly z / eta.  The bar is APPLY_FACTOR = 4 times the float64
    restatement's own distance from the long-double evaluation of the same formula on the device's L, per column; the restatement sums
    over the rows in ascending order, as the kernels document (large_design_cases.apply_restated; test_large_design_host.py shows why
    NumPy's blocked sums are not the measure: against four times THEIR error the device lay at 3.5 and an ascending float64 sum on the CPU
    at 3.2)."""
    n, D, kernel, p = ld.ITER_APPLY
    c, s, ig = tg._iter(n, D, kernel, p, rtol=1e-6)
    L, piv = ig.preconditioner()
    rank, eta = L.shape[1], dc.NUGGET
    assert rank == p
    for name, g1, g2 in ld.apply_probes(n, rank):
        r = te._pieces(ig, g1, g2, p, rtol=1e-6, return_panels=True)
        Z, W = r["z"], r["w"][:, 1:]
        if name == "second segment alone":
            assert not Z[:ld.SEG].any() and Z[ld.SEG:].all()
            assert np.max(np.abs(Z - np.sqrt(eta) * g2)) <= 2. ** -52 * np.sqrt(eta) * np.max(np.abs(g2))
        truth, bar = ld.apply_bar(L, eta, Z)
        frac = ld.apply_fraction(W, truth, bar)
        naive = ld.apply_fraction(Z / eta, truth, bar)
        scale = np.max(np.abs(np.asarray(truth, dtype=np.float64)), axis=0)
        print("n %d %s p %d, %s: w at %.3g of its bar (the bar is %.3g of max|w|); z / eta, what a dropped segment leaves, at %.3g"
              % (n, kernel, p, name, frac.max(), (bar / scale).max(), naive.min()))
        assert not np.array_equal(W, Z / eta) and naive.min() > 1.
        assert frac.max() <= 1.
    ig.close()


def test_estimator_with_the_callers_probes():
    te.test_estimator_with_the_callers_probes(*ld.ITER_LIK)


@pytest.mark.parametrize("n,D,kernel,p", ld.ITER_VAR_SHAPES, ids=lambda v: str(v))
def test_cache_and_bound_against_the_restatement_and_the_exact_variances(n, D, kernel, p):
    tb.test_cache_and_bound_against_the_restatement_and_the_exact_variances(n, D, kernel, p)
    c, (s,) = th.setup(n, D, kernel, m=tb.vh.M_Q)
    ig = tb._iter(c, kernel, p)
    first = ig.variance_bound(c.Xs)
    for mp in (0, 7):
        assert ig.variance_bound(c.Xs, max_points=mp).tobytes() == first.tobytes(), mp
    ig.close()


def test_predict_against_the_dense_predict():
    n, D, kernel, p = ld.ITER_PREDICT
    c, (s,) = th.setup(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    tg._check_against_dense(c, s, kernel, p, gp, ig, c.T[0])
    ig.close()
