"""Host-side checks of the large-design cases (large_design_cases.py): the references alone meet every condition that
test_gpu_large_design.py relies on, at the grid of an MI355X (4 x 256 workgroups).

* the solver's restatement converges within test_iterative_host.ITER_CAP on every shape and column the GPU tests solve at N = 1030 and 4100
  (the GPU tests allow MAX_ITER, so the cap never hides a device failure), the column of the second dot block included;
* with row 1027 moved out, the restatement's pivots start 0, 1027;
* in the failure designs every clean problem is positive definite (accepted by the restatement, cond far below 2^52), every problem of the
  far region singular, and no clean list holds a far point;
* every bar is met by float64 against long double and is not vacuous: local mean and variance, Vecchia terms and gradient rows, the
  Vecchia sum in two orders of addition, the product behind the residual's slack, and the preconditioner's apply evaluated a second way.

Restatement iteration counts, rtol 1e-10, target column: (1030, SE, 64) 25, (1030, UniformMat52, 33) 414, (4100, SE, 40) 116,
(4100, Matern52, 256) 124."""
import math

import numpy as np
import pytest

import dimension_cases as dc
import exact_lik_restate as er
import iterative_restate as ir
import large_design_cases as ld
import local_cases as lc
import local_restate as lr
import test_exact_lik_host as eh
import test_iterative_host as th
import vecchia_cases as vc
import vecchia_restate as vr
from test_iterative_host import ITER_CAP, MAX_ITER, RTOL, SIGMA2

GRID = ld.grid_of(ld.HOST_CUS)
LONG = pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")


def test_shapes_cross_every_size():
    assert GRID == 1024 and ld.local_m(GRID) == 2 * GRID + 37 and ld.vecchia_n(GRID) == 2100
    assert ld.N_DOT == 1030 and ld.N_SEG == 4100 and ld.OUTLIER_ROW >= ld.DOT_BLOCK
    for mp in ld.vecchia_launches(GRID):
        assert mp <= GRID                                        # one problem per workgroup: the path the other tests verify
    for cus in (1, 64, 304):                                     # the rule, whatever the device
        assert ld.grid_of(cus) == 4 * cus
    for bad in (0, -1):
        with pytest.raises(AssertionError, match="could not be read"):
            ld.grid_of(bad)
    src = open(th.ROOT + "/mogp_emulator_amd/csrc/predict_plan.h").read() + open(th.ROOT + "/mogp_emulator_amd/csrc/launch.h").read()
    for text in ("LOCAL_GRID_PER_CU = %d" % ld.LOCAL_GRID_PER_CU, "ITER_SEG = %d" % ld.SEG, "ITER_DOT_BLOCK = %d" % ld.DOT_BLOCK,
                 "VECCHIA_REDUCE_BLOCK = %d" % ld.DOT_BLOCK):
        assert text in src, text


# ---- A. LocalGP ----------------------------------------------------------------------------------------------------------------------------
@LONG
@pytest.mark.parametrize("kernel", ld.LOCAL_KERNELS)
def test_local_float64_lies_inside_the_bars(kernel):
    c, s = ld.local_setup(kernel, GRID)
    ref = ld.local_reference(kernel, GRID)
    rows = np.arange(0, ld.local_m(GRID), 16)
    mean, var, ok, _ = lr.predict(c.X, c.T[0], c.Xs[rows], s, kernel, SIGMA2, dc.NUGGET, ref["nbr"][rows], dtype=np.longdouble)
    em = lc.excess_rows("mean", ref["mean"][rows], np.asarray(mean, dtype=np.float64), ref["cond"][rows])
    ev = lc.excess_rows("var", ref["var"][rows], np.asarray(var, dtype=np.float64), ref["cond"][rows])
    print("%s: float64 mean at %.3g of its bar, variance at %.3g (cond at most %.3g)" % (kernel, em, ev, ref["cond"].max()))
    assert ok.all() and ref["cond"].max() <= 1.2e6 and 0. < em <= 1. and 0. < ev <= 1.


def test_local_failure_design_clean_is_definite_and_far_is_singular():
    X, t, Q, s, n_far = ld.local_failure(GRID)
    k, kernel = ld.LOCAL["k"], ld.LOCAL_FAIL_KERNEL
    nbr, _, _ = lr.neighbours(X, Q, s, k)
    n_clean = ld.LOCAL["N"]
    assert n_far == GRID and Q.shape[0] == ld.local_m(GRID)
    assert np.all(nbr[:GRID] >= n_clean) and np.all(nbr[GRID:] < n_clean)                # a far query sees far points alone, a clean one none
    mean, var, ok, cond = lr.predict(X, t, Q[GRID:], s, kernel, SIGMA2, 0., nbr[GRID:])
    print("clean queries: cond at most %.3g" % cond.max())
    assert ok.all() and cond.max() * k * 2. ** -52 < 1e-3                                # positive definite with room: no rounding refuses it
    far = np.arange(0, GRID, 8)
    _, _, _, cond_far = lr.predict(X, t, Q[far], s, kernel, SIGMA2, 0., nbr[far])
    assert cond_far.min() >= 2. ** 52                                                    # singular: every point beside its copy


# ---- B. Vecchia ----------------------------------------------------------------------------------------------------------------------------
@LONG
@pytest.mark.parametrize("kernel,fit", ld.VECCHIA_CASES)
def test_vecchia_float64_lies_inside_the_bars_and_the_sum_inside_its_bound(kernel, fit):
    N, D, k = ld.vecchia_n(GRID), ld.VECCHIA["D"], ld.VECCHIA["k"]
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, fit)
    ref = ld.vecchia_reference(kernel, fit, GRID)
    order = ref["order"]
    rows = list(range(0, N, 16))
    terms, g, ok, _ = vr.terms(c.X[order], c.T[0][order], s, kernel, sigma2, nugget, ref["nbr"], grad=True, fit_nugget=fit, dtype=np.longdouble, rows=rows)
    et = vc.excess_rows("logpost", ref["terms"][rows], np.asarray(terms[rows], dtype=np.float64), ref["cond"][rows])
    amp = max(1., float(ref["cond"].max()) * 1e-7)
    g64, g80 = ref["grad"][rows].sum(axis=0), np.asarray(g[rows].sum(axis=0), dtype=np.float64)
    eg = dc.excess("grad", g64, g80, amp, max(1., float(np.max(np.abs(g64)))))
    exact, total = math.fsum(ref["terms"]), float(np.sum(np.abs(ref["terms"])))
    bound = (N - 1) * 2. ** -53 * total
    ascending = 0.
    for v in ref["terms"]:
        ascending += v
    es = max(abs(ascending - exact), abs(float(ref["terms"].sum()) - exact)) / bound
    print("%s nugget %s: float64 terms at %.3g of their bar, gradient rows at %.3g, two float64 sums at %.3g of the sum's bound (cond at most %.3g)"
          % (kernel, "fit" if fit else "fixed", et, eg, es, ref["cond"].max()))
    assert ok[rows].all() and amp == 1. and 0. < et <= 1. and 0. < eg <= 1. and es <= 1.
    # a dropped block of 1024 terms is far outside the bound
    assert abs(math.fsum(ref["terms"][ld.DOT_BLOCK:]) - exact) > 1e6 * bound


def test_vecchia_failure_design_clean_is_definite_and_the_copies_are_singular():
    X, t, theta, s, sigma2, clean = ld.vecchia_failure(GRID)
    ref = ld.vecchia_failure_reference(GRID)
    rows, k = ref["rows"], ld.VECCHIA["k"]
    head, nf = ld.VECCHIA_CLEAN_HEAD, ld.VECCHIA_FAR_POINTS
    assert clean[:head].all() and not clean[head:head + 2 * nf].any() and clean[head + 2 * nf:].all()
    lists = ref["nbr"][rows]
    assert np.all(clean[np.maximum(lists, 0)])                                           # no clean list holds a far point
    print("clean points: cond at most %.3g" % ref["cond"][rows].max())
    assert ref["ok"][rows].all() and ref["cond"][rows].max() * (k + 1) * 2. ** -52 < 1e-3
    copies = np.arange(head + nf, head + 2 * nf)
    assert np.all(np.any(ref["nbr"][copies] == (copies - nf)[:, None], axis=1))          # every copy has its original in its list
    _, _, _, cond = vr.terms(X, t, s, ld.VECCHIA_FAIL_KERNEL, sigma2, 0., ref["nbr"], fit_nugget=False, rows=copies[::8])
    assert cond[copies[::8]].min() >= 2. ** 52
    j = copies[0]
    assert not clean[j] and clean[j + GRID]                                              # one grid behind a copy lies a clean point


# ---- C. IterativeGP --------------------------------------------------------------------------------------------------------------------------
def _solve(c, s, kernel, p, B, X=None):
    X = c.X if X is None else X
    K = ir.covariance(X, X, s, kernel, SIGMA2)
    L = ir.pivoted_cholesky(K, p)[0]
    return ir.solve(K + dc.NUGGET * np.eye(K.shape[0]), np.ascontiguousarray(B), L, dc.NUGGET, RTOL, MAX_ITER), K, L


@pytest.mark.parametrize("n,D,kernel,p", ld.ITER_SOLVE_SHAPES, ids=lambda v: str(v))
def test_restatement_converges_within_the_cap(n, D, kernel, p):
    c, s = ld.iter_setup(n, D, kernel)
    cols = [th.right_hand_sides(c, s, kernel)]
    if (n, D, kernel, p) == ld.ITER_TAIL:
        cols.append(ld.tail_column(n))
    if (n, D, kernel, p) in ld.ITER_VAR_SHAPES or (n, D, kernel, p) == ld.ITER_PREDICT:     # the variance's cross columns: every one at 1030, every
        step = 1 if n == ld.N_DOT else 6                                                 # sixth at 4100 (a product costs 16 times as much there)
        cols.append(ir.covariance(c.X, c.Xs[7::step], s, kernel, SIGMA2))
    sv, K, L = _solve(c, s, kernel, p, np.column_stack(cols))
    print("n %d D %d %s p %d: iterations %s" % (n, D, kernel, p, sv.iterations.tolist()))
    assert L.shape[1] == p and sv.converged.all() and 1 <= sv.iterations.min() and sv.iterations.max() <= ITER_CAP
    if (n, D, kernel, p) == ld.ITER_LIK[:2] + (ld.ITER_LIK[3], ld.ITER_LIK[2]):          # the 15 probe columns of the likelihood's pieces
        z = er.probes(L, dc.NUGGET, *eh.caller_probes(n, p, 15))
        sz = ir.solve(K + dc.NUGGET * np.eye(n), z, L, dc.NUGGET, RTOL, MAX_ITER)
        assert sz.converged.all() and sz.iterations.max() <= ITER_CAP


def test_tail_column_is_nonzero_in_the_second_block_alone():
    b = ld.tail_column(ld.N_DOT)
    assert not b[:ld.DOT_BLOCK].any() and np.all(b[ld.DOT_BLOCK:] != 0.) and b.shape == (ld.N_DOT, 1)


def test_outlier_is_the_second_pivot_of_the_restatement():
    n, D, kernel, p = ld.ITER_OUTLIER
    c, s = ld.iter_setup(n, D, kernel)
    X = ld.outlier_design(c.X)
    K = ir.covariance(X, X, s, kernel, SIGMA2)
    L, piv, _ = ir.pivoted_cholesky(K, p)
    assert len(piv) == p and piv[0] == 0 and piv[1] == ld.OUTLIER_ROW
    d = ld.remaining_diagonals(K, L, piv)
    rtol, atol = dc.BARS["fullcov"]
    assert np.all(d[0] == SIGMA2)                                                        # the tie over both blocks
    assert np.all(d.max(axis=1) - d[np.arange(p), piv] <= atol + rtol * SIGMA2)          # the helper finds the restatement's own pivots maximal
    assert d[1, ld.OUTLIER_ROW] - np.delete(d[1], ld.OUTLIER_ROW).max() > 1e3 * (atol + rtol * SIGMA2)     # and the outlier by a wide margin


@LONG
@pytest.mark.parametrize("n,kernel", [(ld.N_DOT, "SquaredExponential"), (ld.N_DOT, "UniformMat52"), (ld.N_SEG, "SquaredExponential")])
def test_float64_product_lies_inside_the_bar_at_these_sizes(n, kernel):
    c, s = ld.iter_setup(n, ld.ITER_D, kernel)
    V = th.matvec_input(n, 4)
    truth = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, dtype=np.longdouble)
    A = ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET)
    bar = th.matvec_bar(np.abs(A), V, ld.ITER_D)
    frac = float(np.max(np.abs(np.asarray((A @ V).astype(np.longdouble) - truth, dtype=np.float64)) / bar))
    print("N %d %s: float64 product at %.3g of the bar" % (n, kernel, frac))
    assert 0. < frac <= 1.


@LONG
def test_float64_apply_evaluated_another_way_lies_inside_its_bar():
    """The bar of the preconditioner's apply is APPLY_FACTOR = 4 times the float64 restatement's own error, and which float64 evaluation
    "the restatement" is matters here: G = eta I + L^T L and L^T z are sums of N = 4100 products, and a chain of N additions in ascending
    order -- what the device's kernels document and what iterative_restate.matvec restates for the product -- rounds several times more
    than NumPy's blocked sums of the same terms.  Measured on the CPU at (4100, SquaredExponential, 40): the ascending-order evaluation
    lies at up to 3.2 (z in the second segment alone) and 1.6 (dense z) times an allowance of 4 times the BLOCKED evaluation's own error, and
    at up to 5.1 over the other kernels and ranks of the issue's table (UniformMat52 40; Matern52 17, 33, 40 and 256; UniformSqExp 40;
    SquaredExponential 17): float64 itself needs more than that allowance at every shape with a second segment, so no choice of shape
    helps.  The restatement the bar is taken from is therefore the ascending-order one; shown here: a second float64 evaluation in that
    order (a factorisation in place of the inverse) and the blocked one both lie inside it, and z / eta is 10^12 bars away."""
    n, D, kernel, p = ld.ITER_APPLY
    c, s = ld.iter_setup(n, D, kernel)
    L = ir.pivoted_cholesky(ir.covariance(c.X, c.X, s, kernel, SIGMA2), p)[0]
    for name, g1, g2 in ld.apply_probes(n, p):
        Z = er.probes(L, dc.NUGGET, g1, g2)
        truth, bar = ld.apply_bar(L, dc.NUGGET, Z)
        other = ld.apply_fraction(ld.apply_restated(L, dc.NUGGET, Z, how="factorised"), truth, bar)
        blocked = ld.apply_fraction(ld.apply_restated(L, dc.NUGGET, Z, how="blocked"), truth, bar)
        scale = np.max(np.abs(np.asarray(truth, dtype=np.float64)), axis=0)
        dropped = ld.apply_fraction(Z / dc.NUGGET, truth, bar)                           # what a dropped second segment gives in the first case
        print("%s: bar %.3g of max|w|; float64 in ascending order by a factorisation at %.3g of it, NumPy's blocked sums at %.3g; z / eta at %.3g"
              % (name, (bar / scale).max(), other.max(), blocked.max(), dropped.min()))
        assert np.all(bar > 0.) and other.max() <= 1. and blocked.max() <= 1.
        if name == "second segment alone":
            assert not Z[:ld.SEG].any() and Z[ld.SEG:].all() and dropped.min() > 1e6
