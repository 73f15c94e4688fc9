"""Iterative exact prediction on the MI355X (mogp_emulator_amd.IterativeGP, csrc/kernels_iter.hip, csrc/engine_iter.hip) against the NumPy
restatement (iterative_restate.py) and the dense GaussianProcessGPU.predict, at the smallest shapes where the code can go another way: one,
a partial and several blocks of 16 right-hand sides, a second panel of 32 (r = 33), designs of two to sixteen row tiles with a partial last
one, every kernel, both ends of the input dimension, both query counts of dimension_cases, preconditioner ranks from none to 256.  Every design here fits one block of 1024 rows of the dots and of
the pivot search and one segment of 4096 rows of the preconditioner: N > 1024 (1030 and 4100) is in test_gpu_large_design.py.

The shapes, the right-hand sides and the product's bar are those of test_iterative_host.py, which shows on the CPU that the restatement
converges within 600 iterations where these tests allow 1000, and that the bar is neither vacuous nor missed by float64.  Hyperparameters
come from dimension_cases.case (fixed nugget 1e-4, sigma^2 = e^0.1).  Measured figures are printed as fractions of their bars; DESIGN.md
section 3 "Iterative exact prediction" records them."""
import functools
import importlib

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import iterative_restate as ir
import test_iterative_host as th
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")
SUB = 64          # the emulator the hyperparameters come from is fitted on the first rows only: IterativeGP must not look at its data


def _gp(X, t, kernel, theta, nugget=dc.NUGGET, mean=None):
    D = X.shape[1]
    gp = M.GaussianProcessGPU(X, t, mean=mean, kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=dc.n_corr(kernel, D), nugget_type="fixed"))
    gp.fit(theta)
    return gp


def _iter(n, D, kernel, p, m=dc.M_TEST[0], **kw):
    c, (s,) = th.setup(n, D, kernel, m=m)
    gp = _gp(c.X[:min(SUB, n)], c.T[0, :min(SUB, n)], kernel, c.thetas[0])
    kw.setdefault("rtol", RTOL)
    kw.setdefault("max_iter", MAX_ITER)
    return c, s, M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, **kw)


@functools.lru_cache(maxsize=None)
def _dense(n, D, kernel):
    """(A float64, A long double, eigenvalues, cond, amp) of one shape, computed once and never changed"""
    c, (s,) = th.setup(n, D, kernel)
    A = ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET)
    A80 = ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET, dtype=np.longdouble)
    cond, amp = dc.amplification(A)
    for a in (A, A80):
        a.setflags(write=False)
    return A, A80, cond, amp


def _fraction_of_bar(got, truth80, bar):
    return float(np.max(np.abs(np.asarray(got.astype(np.longdouble) - truth80, dtype=np.float64)) / bar))


# ---- the product ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,r,kernel", th.MATVEC_CASES, ids=lambda v: str(v))
def test_matvec_against_the_restatement(N, D, r, kernel):
    c, s, ig = _iter(N, D, kernel, 0)
    V = th.matvec_input(N, r)
    got = ig.matvec(V)
    ig.close()
    assert got.shape == (N, r)
    truth = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, dtype=np.longdouble)
    bar = th.matvec_bar(np.abs(ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET)), V, D)
    frac = _fraction_of_bar(got, truth, bar)
    print("N %d D %d r %d %s: product at %.3g of its bar" % (N, D, r, kernel, frac))
    assert frac <= 1.


@pytest.mark.parametrize("kernel", th.FOUR)
@pytest.mark.parametrize("m", dc.M_TEST)
@pytest.mark.parametrize("N,D,r", [(130, 3, 16), (300, 3, 7)])
def test_rectangular_matvec_against_the_restatement(N, D, r, m, kernel):
    c, s, ig = _iter(N, D, kernel, 0, m=m)
    V = th.matvec_input(N, r)
    got = ig.matvec(V, testing=c.Xs)
    again = ig.matvec(V, testing=c.Xs)
    one = ig.matvec(V, testing=c.Xs[5:6])
    ig.close()
    assert got.shape == (m, r) and np.array_equal(got, again) and np.array_equal(one[0], got[5])      # a row depends on its query alone
    truth = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, Q=c.Xs, dtype=np.longdouble)
    bar = th.matvec_bar(np.abs(ir.covariance(c.Xs, c.X, s, kernel, SIGMA2)), V, D)
    frac = _fraction_of_bar(got, truth, bar)
    print("N %d D %d r %d m %d %s: rectangular product at %.3g of its bar" % (N, D, r, m, kernel, frac))
    assert frac <= 1.


def test_matvec_is_reproducible_and_its_columns_are_independent():
    N, D, kernel = 300, 3, "Matern52"
    c, s, ig = _iter(N, D, kernel, 0)
    V = th.matvec_input(N, 33)
    first = ig.matvec(V)
    assert np.array_equal(ig.matvec(V), first)
    for j in (0, 7, 15, 16, 31, 32):
        assert np.array_equal(ig.matvec(V[:, j]), first[:, j]), j
        assert np.array_equal(ig.matvec(V[:, [j]])[:, 0], first[:, j]), j
    assert np.array_equal(ig.matvec(V[:, 5:22]), first[:, 5:22])
    ig.close()


# ---- the preconditioner -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,kernel,p", [s for s in th.SOLVE_SHAPES if s[3] > 0], ids=lambda v: str(v))
def test_preconditioner_against_the_restatement_on_the_devices_pivots(n, D, kernel, p):
    c, s, ig = _iter(n, D, kernel, p)
    L, piv = ig.preconditioner()
    L2, piv2 = ig.preconditioner()
    ig.close()
    rank = len(piv)
    assert L.shape == (n, rank) and rank <= p and np.array_equal(L, L2) and np.array_equal(piv, piv2)
    assert piv[0] == 0                                         # the diagonal is constant: ties go to the lowest index
    assert len(set(piv.tolist())) == rank and piv.min() >= 0 and piv.max() < n
    if (n, D) == (130, 1):
        assert rank < p                                        # the remaining diagonal runs out: the rank stops early
    else:
        assert rank == p
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    want, piv_r, left = ir.pivoted_cholesky(K, rank, pivots=piv)
    r = len(piv_r)
    rtol, atol = dc.BARS["fullcov"]
    # Where the rank stops early the last pivots are rounding noise: the restatement, on the device's own pivots, may find a remaining
    # diagonal <= 0 a few steps before the device does.  The columns both have are compared; at the first pivot the restatement refuses,
    # its remaining diagonal must be zero to the bar (the device's positive value there is then within the bar of it).
    assert r == rank or ((n, D) == (130, 1) and r >= rank - 4)
    _, amp = dc.amplification(K[np.ix_(piv[:r], piv[:r])])     # the pivot block is what the columns are divided through
    if r < rank:
        assert abs(left[piv[r]]) <= amp * (atol + rtol * SIGMA2)
    e = dc.excess("fullcov", L[:, :r], want, amp)
    # the device's columns behind those: compared against nothing above, so what they add to any row of L L^T must itself be within the bar
    tail = float(np.max(np.sum(L[:, r:] ** 2, axis=1))) if r < rank else 0.
    assert tail <= amp * (atol + rtol * SIGMA2), tail
    slack = float(np.min(SIGMA2 - np.sum(L * L, axis=1)))
    print("n %d D %d %s p %d: rank %d (restatement on the same pivots %d), L at %.3g of its bar (amplification %.3g), smallest remaining diagonal %.3g, "
          "columns behind the restatement's add at most %.3g" % (n, D, kernel, p, rank, r, e, amp, slack, tail))
    assert e <= 1.
    assert slack >= -amp * (atol + rtol * SIGMA2)


def test_preconditioner_cuts_the_iterations():
    n, D, kernel = 300, 3, "SquaredExponential"
    c, s, plain = _iter(n, D, kernel, 0)
    _, _, pre = _iter(n, D, kernel, 64)
    a, b = plain.solve(c.T[0]), pre.solve(c.T[0])
    plain.close()
    pre.close()
    print("iterations without / with a rank-64 preconditioner: %d / %d (14 against 598 on the CPU)" % (a.iterations[0], b.iterations[0]))
    assert a.converged.all() and b.converged.all() and a.precond_rank == 0 and b.precond_rank == 64
    assert b.iterations[0] < a.iterations[0]


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------
def _host_residual(A80, B, x):
    r = B.astype(np.longdouble) - A80 @ x.astype(np.longdouble)
    return np.asarray(np.sqrt(np.sum(r * r, axis=0)), dtype=np.float64) / np.linalg.norm(B, axis=0)


def _residual_slack(A, B, x, D, res):
    """what the device's |b - A x| / |b| may differ by from the host's: the product's bar on A x, and the fixed-order sum of N squares"""
    N = A.shape[0]
    return np.linalg.norm(th.matvec_bar(np.abs(A), x, D), axis=0) / np.linalg.norm(B, axis=0) + (N + 4) * 2. ** -52 * res


@pytest.mark.parametrize("n,D,kernel,p", th.SOLVE_SHAPES, ids=lambda v: str(v))
def test_solve_converges_and_reports_its_true_residual(n, D, kernel, p):
    c, s, ig = _iter(n, D, kernel, p)
    A, A80, cond, amp = _dense(n, D, kernel)
    B = th.right_hand_sides(c, s, kernel)
    sv = ig.solve(B)
    again = ig.solve(B)
    assert sv.x.shape == B.shape and sv.iterations.shape == sv.residual.shape == sv.converged.shape == (8,)
    assert np.array_equal(sv.x, again.x) and np.array_equal(sv.iterations, again.iterations) and np.array_equal(sv.residual, again.residual)
    host = _host_residual(A80, B, sv.x)
    print("n %d D %d %s p %d: rank %d, iterations %s, residual at most %.3g (host %.3g), cond %.3g"
          % (n, D, kernel, p, sv.precond_rank, sv.iterations.tolist(), sv.residual.max(), host.max(), cond))
    assert sv.converged.all() and sv.iterations.max() <= MAX_ITER and sv.iterations.min() >= 1
    assert np.all(np.abs(sv.residual - host) <= _residual_slack(A, B, sv.x, D, host))
    # every column is its own problem, bit for bit and iteration for iteration
    for j in (0, 3, 7):
        one = ig.solve(B[:, [j]])
        assert np.array_equal(one.x[:, 0], sv.x[:, j]) and one.iterations[0] == sv.iterations[j], j
        assert one.residual[0] == sv.residual[j] and one.converged[0] == sv.converged[j], j
    vec = ig.solve(B[:, 0])
    assert vec.x.shape == (n,) and np.array_equal(vec.x, sv.x[:, 0])
    ig.close()


@pytest.mark.parametrize("n,D,kernel,p", th.SOLVE_SHAPES, ids=lambda v: str(v))
def test_reported_residual_stays_within_the_drift_bound(n, D, kernel, p):
    """residual <= rtol (1 + cond(A) N 2^-52): how far the recomputed residual of a converged column may lie above rtol.

    The bound leaves next to nothing for the gap between the recurrence residual, which freezes a column, and the true one, which is
    reported: that gap is additive and does not shrink with rtol.  With x updated by a plain fused multiply-add the target column of
    (1000, 5, UniformSqExp, p = 128) reported 1.00421e-10 on an MI355X -- a gap of 2.8e-12 |b|, roundings of the size of x in every late
    step -- and missed the bound; with the iterate carried as a compensated sum (cg_update_kernel) it reports 9.7626e-11, and the largest
    figure over the eight shapes is 9.96e-11.  Measured: DESIGN.md section 3."""
    c, s, ig = _iter(n, D, kernel, p)
    A, A80, cond, amp = _dense(n, D, kernel)
    sv = ig.solve(th.right_hand_sides(c, s, kernel))
    ig.close()
    print("n %d D %d %s p %d: residual %s, bound %.17g" % (n, D, kernel, p, sv.residual, RTOL * (1. + cond * n * 2. ** -52)))
    assert sv.converged.all()
    assert np.all(sv.residual <= RTOL * (1. + cond * n * 2. ** -52))


def test_solve_of_more_columns_than_one_block_and_of_a_zero_column():
    n, D, kernel, p = 300, 3, "SquaredExponential", 64
    c, s, ig = _iter(n, D, kernel, p, m=dc.M_TEST[0])
    B = np.ascontiguousarray(np.column_stack([c.T[0], ir.covariance(c.X, c.Xs[:34], s, kernel, SIGMA2)]))      # 35 columns: 32 + 3
    B[:, 4] = 0.
    sv = ig.solve(B)
    assert sv.converged.all() and sv.iterations[4] == 0 and sv.residual[4] == 0. and not sv.x[:, 4].any()
    for j in (0, 4, 31, 32, 34):
        one = ig.solve(B[:, [j]])
        assert np.array_equal(one.x[:, 0], sv.x[:, j]) and one.iterations[0] == sv.iterations[j], j
    ig.close()


def test_a_solve_that_does_not_converge_is_reported_not_raised():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, s, ig = _iter(n, D, kernel, p, max_iter=3)
    A, A80, cond, amp = _dense(n, D, kernel)
    B = th.right_hand_sides(c, s, kernel)
    sv = ig.solve(B)
    ig.close()
    host = _host_residual(A80, B, sv.x)
    print("max_iter 3: residual %s" % sv.residual)
    assert not sv.converged.any() and np.all(sv.iterations == 3) and np.all(np.isfinite(sv.x))
    assert np.all(np.abs(sv.residual - host) <= _residual_slack(A, B, sv.x, D, host)) and np.all(sv.residual > RTOL)


# ---- the prediction ------------------------------------------------------------------------------------------------------------------------
def _check_against_dense(c, s, kernel, p_rank, gp, ig, y_resid, shift=0.):
    n, D = c.X.shape
    A, A80, cond, amp = _dense(n, D, kernel)
    dense = gp.predict(c.Xs, deriv=False)
    pr = ig.predict(c.Xs, unc=True)
    assert pr.mean.shape == pr.unc.shape == pr.var_converged.shape == pr.var_residual.shape == (c.Xs.shape[0],)
    assert bool(pr.converged) and pr.var_converged.all() and pr.iterations >= 1
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)           # (n, m)
    w = np.linalg.solve(A, ks)                                 # A^-1 k*
    wn, kn = np.linalg.norm(w, axis=0), np.linalg.norm(ks, axis=0)
    rho = np.linalg.norm(y_resid - A @ ig.weights())           # exact algebra for an inexact alpha: |k*^T (alpha - A^-1 y)| <= |A^-1 k*| |rho|
    rt, at = dc.BARS["mean"]
    mean_bar = amp * (at + rt * np.abs(dense.mean)) + wn * rho
    rt, at = dc.BARS["var"]
    var_bar = amp * (at + rt * np.abs(dense.unc)) + wn * pr.var_residual * kn
    em, ev = float(np.max(np.abs(pr.mean - dense.mean) / mean_bar)), float(np.max(np.abs(pr.unc - dense.unc) / var_bar))
    print("n %d D %d %s p %d: mean at %.3g of its bar, variance at %.3g (alpha: %d iterations, residual %.3g; cond %.3g)"
          % (n, D, kernel, p_rank, em, ev, pr.iterations, pr.residual, cond))
    assert em <= 1. and ev <= 1.
    return pr


@pytest.mark.parametrize("n,D,kernel,p", th.PREDICT_SHAPES, ids=lambda v: str(v))
def test_predict_against_the_dense_predict(n, D, kernel, p):
    c, (s,) = th.setup(n, D, kernel)
    gp = _gp(c.X, c.T[0], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    pr = _check_against_dense(c, s, kernel, p, gp, ig, c.T[0])
    # the nugget in the variance, and the mean without the variance
    nn = ig.predict(c.Xs, unc=True, include_nugget=False)
    assert np.array_equal(nn.mean, pr.mean) and np.all(nn.unc < pr.unc)
    bare = ig.predict(c.Xs)
    assert bare.unc is None and bare.var_converged is None and bare.var_residual is None and np.array_equal(bare.mean, pr.mean)
    ig.close()


def test_predict_does_not_depend_on_the_passes_or_on_the_other_queries():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, s, ig = _iter(n, D, kernel, p)
    m = c.Xs.shape[0]

    def bits(q):
        return [q.mean.tobytes(), q.unc.tobytes(), q.var_converged.tobytes(), q.var_residual.tobytes()]
    first = ig.predict(c.Xs, unc=True)
    assert bits(ig.predict(c.Xs, unc=True)) == bits(first)
    for mp in (1, 7, m):
        assert bits(ig.predict(c.Xs, unc=True, max_points=mp)) == bits(first), mp
    for j in (0, 5, 33, m - 1):
        one = ig.predict(c.Xs[j:j + 1], unc=True)
        assert (one.mean[0].tobytes(), one.unc[0].tobytes(), one.var_residual[0].tobytes()) == (
            first.mean[j].tobytes(), first.unc[j].tobytes(), first.var_residual[j].tobytes()), j
    ig.close()


def test_multi_output_rows_are_the_single_emulator_calls():
    n, D, kernel, p, E, nq = th.MULTI
    c, scales = th.setup(n, D, kernel, E=E)
    mo = M.MultiOutputGP_GPU(c.X[:SUB], c.T[:, :SUB], kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=c.nc, nugget_type="fixed"))
    mo.fit(c.thetas)
    ig = M.IterativeGP(mo, c.X, c.T, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    pr = ig.predict(c.Xs[:nq], unc=True)
    assert pr.mean.shape == pr.unc.shape == pr.var_converged.shape == pr.var_residual.shape == (E, nq)
    assert pr.converged.shape == pr.residual.shape == pr.iterations.shape == (E,) and pr.converged.all()
    V = th.matvec_input(n, 3)
    for e in range(E):
        ge = _gp(c.X[:SUB], c.T[e, :SUB], kernel, c.thetas[e])
        one = M.IterativeGP(ge, c.X, c.T[e], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        q = one.predict(c.Xs[:nq], unc=True)
        assert np.array_equal(q.mean, pr.mean[e]) and np.array_equal(q.unc, pr.unc[e]) and np.array_equal(q.var_residual, pr.var_residual[e])
        assert q.iterations == pr.iterations[e] and q.residual == pr.residual[e]
        assert np.array_equal(one.weights(), ig.weights(emulator=e)) and np.array_equal(one.matvec(V), ig.matvec(V, emulator=e))
        one.close()
    assert not np.array_equal(pr.mean[0], pr.mean[1]) and not np.array_equal(pr.unc[1], pr.unc[2])
    ig.close()


def test_fixed_linear_mean_is_subtracted_and_added_back():
    n, D, kernel, p, beta = th.LINEAR_MEAN                     # c + c x[0], its coefficients fixed in theta
    c, (s,) = th.setup(n, D, kernel)
    gp = _gp(c.X, c.T[0], kernel, np.r_[beta, c.thetas[0]], mean=LibGPGPU.PolyMeanFunc([[0, 1]]))
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    resid = c.T[0] - (beta[0] + beta[1] * c.X[:, 0])
    pr = _check_against_dense(c, s, kernel, p, gp, ig, resid)
    ig.close()
    zero = _gp(c.X, c.T[0], kernel, c.thetas[0])
    plain = M.IterativeGP(zero, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER).predict(c.Xs)
    assert np.max(np.abs(pr.mean - plain.mean)) > 1e-6        # the mean function matters on these data


def test_vecchia_predict_exact_is_iterative_gp_on_the_same_handle_data():
    n, D, kernel, p = 300, 3, "SquaredExponential", 64
    c, (s,) = th.setup(n, D, kernel)
    A, A80, cond, amp = _dense(n, D, kernel)
    gp = _gp(c.X[:SUB], c.T[0, :SUB], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    want, alpha = ig.predict(c.Xs, unc=True), ig.weights()
    ig.close()
    kw = dict(precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    # the caller's order kept: the same data on the handle, hence the same bits
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, order=np.arange(n))
    with pytest.raises(RuntimeError, match="fit has not been called and no theta was given"):
        vg.predict_exact(c.Xs)
    got = vg.predict_exact(c.Xs, theta=c.thetas[0], unc=True, **kw)
    assert np.array_equal(got.mean, want.mean) and np.array_equal(got.unc, want.unc) and got.iterations == want.iterations
    assert np.array_equal(vg.weights_in_callers_order(vg.exact_view(c.thetas[0], **kw)), alpha)
    vg.close()
    # a random order: another order of every sum, the same posterior; the weights come back in the caller's numbering
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, rng=3)
    assert not np.array_equal(vg.order, np.arange(n))
    got = vg.predict_exact(c.Xs, theta=c.thetas[0], unc=True, **kw)
    a2 = vg.weights_in_callers_order(vg.exact_view(c.thetas[0], **kw))
    vg.close()
    ev = np.linalg.eigvalsh(A)
    ynorm = np.linalg.norm(c.T[0])
    assert bool(got.converged) and got.var_converged.all()
    assert np.linalg.norm(a2 - alpha) <= (got.residual + want.residual) * ynorm / ev[0] * (1. + 1e-6)
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    wn, kn = np.linalg.norm(np.linalg.solve(A, ks), axis=0), np.linalg.norm(ks, axis=0)
    rt, at = dc.BARS["mean"]
    assert np.all(np.abs(got.mean - want.mean) <= amp * (at + rt * np.abs(want.mean)) + wn * (got.residual + want.residual) * ynorm)
    rt, at = dc.BARS["var"]
    assert np.all(np.abs(got.unc - want.unc) <= amp * (at + rt * np.abs(want.unc)) + wn * (got.var_residual + want.var_residual) * kn)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work(monkeypatch):
    from test_local_host import _fake_gp
    created = []

    def no_device(inputs, residuals, device):
        created.append(inputs.shape)
        raise AssertionError("the device must not be reached")
    n, D, kernel = 130, 3, "SquaredExponential"
    c, (s,) = th.setup(n, D, kernel)
    X, t = c.X, c.T[0]
    real = _gp(X[:SUB], t[:SUB], kernel, c.thetas[0])
    zero_nugget = _gp(X[:SUB], t[:SUB], kernel, c.thetas[0], nugget=0.)
    monkeypatch.setattr(IG, "_create_native", no_device)
    for kw, msg in ((dict(nugget_type="pivot"), 'IterativeGP: not available with nugget="pivot"'),
                    (dict(analytic=True), "IterativeGP: not available with analytic_mean=True"),
                    (dict(fit=False), "IterativeGP: hyperparameters have not been fit for this Gaussian Process"),
                    (dict(kernel="ProductMat52"), "IterativeGP: not available with the ProductMat52 kernel")):
        with pytest.raises(RuntimeError, match=msg):
            M.IterativeGP(_fake_gp(**kw), X, t)
    with pytest.raises(ValueError, match=r"IterativeGP: the nugget must be positive \(the preconditioner divides by it\)"):
        M.IterativeGP(zero_nugget, X, t, precond_rank=8)
    for p in (-1, 131, 2.5):
        with pytest.raises(ValueError, match=r"IterativeGP: precond_rank must be between 0 and min\(N, 1024\) = 130"):
            M.IterativeGP(real, X, t, precond_rank=p)
    for r in (0., 1., -1e-8, np.nan):
        with pytest.raises(ValueError, match="IterativeGP: rtol must lie between 0 and 1"):
            M.IterativeGP(real, X, t, precond_rank=8, rtol=r)
    for it in (0, -2, 1.5):
        with pytest.raises(ValueError, match="IterativeGP: max_iter must be at least 1"):
            M.IterativeGP(real, X, t, precond_rank=8, max_iter=it)
    for b in (np.zeros((n, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):       # D != gp.D among them
        with pytest.raises(ValueError, match="IterativeGP: inputs must have shape"):
            M.IterativeGP(real, b, t, precond_rank=8)
    for bad_t in (np.zeros(n - 1), np.zeros((2, n)), np.zeros((n, 1))):
        with pytest.raises(ValueError, match="IterativeGP: targets must have shape"):
            M.IterativeGP(real, X, bad_t, precond_rank=8)
    for v in (np.nan, np.inf):
        Xb, tb = X.copy(), t.copy()
        Xb[2, 1], tb[3] = v, v
        with pytest.raises(ValueError, match="IterativeGP: inputs must be finite"):
            M.IterativeGP(real, Xb, t, precond_rank=8)
        with pytest.raises(ValueError, match="IterativeGP: targets must be finite"):
            M.IterativeGP(real, X, tb, precond_rank=8)
    with pytest.raises(ValueError, match="IterativeGP: device must be"):
        M.IterativeGP(real, X, t, precond_rank=8, device=-1)
    assert created == []
    monkeypatch.undo()
    # the native layer refuses by name too (a caller of the C ABI has no Python in front of it)
    ig = M.IterativeGP(real, X, t, precond_rank=8)
    kt, sc, sigma2, nugget = ig._hyper[0][:4]
    with pytest.raises(RuntimeError, match="solve: precondition has not been called"):
        ig._native.solve(t[:, None], 1e-8, 10)
    with pytest.raises(RuntimeError, match=r"precondition: precond_rank must be between 0 and min\(N, 1024\) = 130"):
        ig._native.precondition(kt, sc, sigma2, nugget, 131)
    with pytest.raises(RuntimeError, match="precondition: the nugget must be positive"):
        ig._native.precondition(kt, sc, sigma2, 0., 8)
    ig._native.precondition(kt, sc, sigma2, nugget, 8)
    with pytest.raises(RuntimeError, match="solve: rtol must lie between 0 and 1"):
        ig._native.solve(t[:, None], 1., 10)
    with pytest.raises(RuntimeError, match="solve: max_iter must be at least 1"):
        ig._native.solve(t[:, None], 1e-8, 0)
    with pytest.raises(ValueError, match="IterativeGP.predict: testing must have shape"):
        ig.predict(np.zeros((4, 2)))
    ig.close()
    with pytest.raises(RuntimeError, match="has been closed"):
        ig.solve(t)
