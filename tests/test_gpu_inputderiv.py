"""Input derivatives at large designs on the MI355X (mogp_emulator_amd.IterativeGP.matvec_inputderiv, predict(deriv=True),
PosteriorPaths.gradient; csrc/kernels_iter.hip kinderiv_kernel, csrc/kernels_rff.hip rff_inderiv_kernel) against the NumPy restatement
(inputderiv_restate.py) in long double and the dense GaussianProcessGPU.predict(deriv=True), at the smallest shapes where the kernels can go
another way: one, a partial and several tiles of 64 queries, of 64 design points and of 64 features, one and two MFMA blocks of 16 columns and
a second pass of 32, dimensions on both sides of the groups of 8 (and D = 80 once per kernel), designs away from the origin.

The bars are those of inputderiv_restate.py; test_inputderiv_host.py shows on the CPU that float64 in the difference form meets them and that
the expanded form and float32 frequencies miss them.  Measured figures are printed as fractions of their bars; DESIGN.md section 3 "Input
derivatives at large designs" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import inputderiv_restate as idr
import iterative_restate as ir
import pathwise_restate as pw
import test_gpu_iterative as tg
import test_inputderiv_host as ih
import test_iterative_host as th
import test_pathwise_host as ph
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu

ETA = dc.NUGGET
F_SMALL = 64
SE, M52 = "SquaredExponential", "Matern52"
# (kernel, M queries, N, D, c columns, shift) of the kernel-derivative sweep: the four kernels at (130, 3); D on both sides of every multiple of
# the group of 8 up to 17, with M in {1, 37, 65, 130} and c in {1, 7, 16, 17, 33} in turn; D = 80 once per kernel; N in {1, 126, 300, 1030};
# the shifted designs of the host test
SWEEP_CASES = ([(k, 37, 130, 3, 7, 0.) for k in th.FOUR]
               + [(SE, 1, 130, 1, 33, 0.), (M52, 37, 130, 2, 1, 0.), (SE, 65, 130, 4, 7, 0.), (M52, 130, 130, 5, 16, 0.), (SE, 1, 130, 7, 17, 0.),
                  (M52, 37, 130, 8, 33, 0.), (SE, 65, 130, 9, 1, 0.), (M52, 130, 130, 16, 7, 0.), (SE, 37, 130, 17, 16, 0.), (M52, 65, 130, 17, 17, 0.)]
               + [(SE, 65, 130, 80, 16, 0.), (M52, 37, 126, 80, 17, 0.)]
               + [(M52, 130, 1, 3, 1, 0.), (SE, 65, 126, 2, 33, 0.), (SE, 130, 300, 3, 17, 0.), (M52, 37, 1030, 5, 16, 0.)]
               + ih.SHIFTED_CASES)
# (Mq, N, D, F, S, kernel) of the feature derivative: the feature product's cases (F in {1, 3, 64, 65, 130, 256}, D in {1, 3, 17, 80}) and
# dimensions around the groups of 8
FEATURE_CASES = ph.PRODUCT_CASES + [(37, 130, 2, 1, 1, M52), (65, 130, 4, 64, 7, SE), (1, 130, 5, 65, 16, M52), (37, 130, 7, 130, 17, SE),
                                    (65, 130, 8, 64, 33, M52), (130, 130, 9, 65, 17, SE), (37, 130, 16, 130, 16, M52)]


def _kt(kernel):
    return 1 if kernel in ir.MATERN else 0


def _amp(F):
    return np.sqrt(2. * SIGMA2 / F)


# ---- the two products ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,Mq,N,D,c,shift", SWEEP_CASES, ids=lambda v: str(v))
def test_kernel_derivative_sweep_against_the_long_double_restatement(kernel, Mq, N, D, c, shift):
    X, Q, s, V, cs = ih.sweep_inputs(kernel, Mq, N, D, c, shift)
    native = LibGPGPU.LocalGP_GPU(X, cs.T[:1])
    got = native.kmatvec_inputderiv(_kt(kernel), s, SIGMA2, V, Q)
    native.close()
    assert got.shape == (Mq, D, c)
    Qt, Xt = ir.scaled(Q, s), ir.scaled(X, s)
    truth = idr.kgrad_in(Qt, Xt, s, kernel, SIGMA2, V, dtype=np.longdouble)
    frac = ih.fraction_of_bar(got, truth, idr.kgrad_bar(Qt, Xt, s, kernel, SIGMA2, V))
    print("%s M %d N %d D %d c %d shift %g: kernel-derivative sweep at %.3g of its bar" % (kernel, Mq, N, D, c, shift, frac))
    assert frac <= 1.


@pytest.mark.parametrize("Mq,N,D,F,S,kernel", FEATURE_CASES, ids=lambda v: str(v))
def test_feature_derivative_against_the_long_double_restatement(Mq, N, D, F, S, kernel):
    Pt, s, raw, c, omega, phase, W = ph.product_inputs(Mq, N, D, F, S, kernel)
    native = LibGPGPU.LocalGP_GPU(c.X, c.T[:1])
    got = native.rff_inputderiv(s, omega, phase, W, _amp(F), c.X if raw is None else raw)
    native.close()
    assert got.shape == (S, Pt.shape[0], D)
    truth = idr.rff_grad(Pt, s, omega, phase, W, SIGMA2, dtype=np.longdouble)
    frac = ih.fraction_of_bar(np.transpose(got, (1, 2, 0)), truth, idr.rffgrad_bar(Pt, s, omega, phase, W, SIGMA2))
    print("M %d D %d F %d S %d %s: feature derivative at %.3g of its bar" % (Pt.shape[0], D, F, S, kernel, frac))
    assert frac <= 1.


# ---- bit for bit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,D", [(M52, 3), (SE, 9)])
def test_sweep_is_reproducible_and_its_rows_columns_and_passes_are_independent(kernel, D):
    Mq, N, c = 130, 130, 33
    X, Q, s, V, cs = ih.sweep_inputs(kernel, Mq, N, D, c)
    V[:, 4] = 0.
    c0, s0, ig = tg._iter(N, D, kernel, 0, m=Mq)
    assert np.array_equal(c0.X, X) and np.array_equal(c0.Xs, Q)
    first = ig.matvec_inputderiv(V, Q)
    assert first.shape == (Mq, D, c) and np.array_equal(ig.matvec_inputderiv(V, Q), first)
    assert np.array_equal(ig._native.kmatvec_inputderiv(_kt(kernel), s, SIGMA2, V, Q), first)
    assert not first[:, :, 4].any() and first[:, :, 3].any()                     # a zero column gives exact zeros
    for mp in (1, 64, 100):
        assert np.array_equal(ig.matvec_inputderiv(V, Q, max_points=mp), first), mp
    for i in (0, 63, 64, 129):
        assert np.array_equal(ig.matvec_inputderiv(V, Q[i:i + 1])[0], first[i]), i
    for j in (0, 7, 15, 16, 31, 32):
        one = ig.matvec_inputderiv(V[:, j], Q)
        assert one.shape == (Mq, D) and np.array_equal(one, first[:, :, j]), j
        assert np.array_equal(ig.matvec_inputderiv(V[:, [j]], Q)[:, :, 0], first[:, :, j]), j
    assert np.array_equal(ig.matvec_inputderiv(V[:, 5:22], Q), first[:, :, 5:22])
    # a query on a design point: an exact zero from that point, and the other points' sum untouched by it
    on = ig.matvec_inputderiv(V, X[:70])
    Vz = V.copy()
    for i in (0, 69):
        Vz[:] = V
        Vz[i] = 0.
        assert np.array_equal(ig.matvec_inputderiv(Vz, X[i:i + 1])[0], on[i]), i
    ig.close()


@pytest.mark.parametrize("kernel", [SE, M52])
def test_one_design_point_under_the_query_gives_exact_zeros(kernel):
    x = np.array([[0.3, 0.7, 0.2]])
    s = np.array([1.7, 0.4, 2.2])
    native = LibGPGPU.LocalGP_GPU(x, np.ones((1, 1)))
    got = native.kmatvec_inputderiv(_kt(kernel), s, SIGMA2, np.array([[1.5, -2.]]), np.vstack([x, x + 0.1]))
    native.close()
    assert got.shape == (2, 3, 2) and np.all(got[0] == 0.) and np.all(np.isfinite(got)) and np.all(got[1] != 0.)


def test_feature_derivative_is_reproducible_and_its_rows_columns_and_passes_are_independent():
    Mq, N, D, F, S, kernel = 130, 130, 9, 130, 33, M52
    Pt, s, raw, c, omega, phase, W = ph.product_inputs(Mq, N, D, F, S, kernel)
    W[4] = 0.
    native = LibGPGPU.LocalGP_GPU(c.X, c.T[:1])
    first = native.rff_inputderiv(s, omega, phase, W, _amp(F), raw)
    assert first.shape == (S, Mq, D) and np.array_equal(native.rff_inputderiv(s, omega, phase, W, _amp(F), raw), first)
    assert not first[4].any() and first[3].any()
    for j in (0, 7, 15, 16, 31, 32):
        assert np.array_equal(native.rff_inputderiv(s, omega, phase, W[j:j + 1], _amp(F), raw)[0], first[j]), j
    assert np.array_equal(native.rff_inputderiv(s, omega, phase, W[5:22], _amp(F), raw), first[5:22])
    for i in (0, 63, 64, 129):
        assert np.array_equal(native.rff_inputderiv(s, omega, phase, W, _amp(F), raw[i:i + 1])[:, 0], first[:, i]), i
    for mp in (1, 64, 100):
        assert np.array_equal(native.rff_inputderiv(s, omega, phase, W, _amp(F), raw, max_points=mp), first), mp
    native.close()


# ---- the paths ----------------------------------------------------------------------------------------------------------------------------
def _path_bars(c, s, kernel, paths, Q, dmean):
    """(truth (S, m, D) long double, bar of the prior's gradient, bar of the whole): the two product bars and the rounding of the two sums
    (the mean function's derivative, then the kernel part: each rounded sum is off by at most 2^-53 of its result)"""
    Qt, Xt = ir.scaled(Q, s), ir.scaled(c.X, s)
    W, v = paths.feature_normals, paths.update
    truth_prior = np.transpose(idr.rff_grad(Qt, s, paths.omega, paths.phase, W, SIGMA2, dtype=np.longdouble), (2, 0, 1))
    if dmean is not None:
        truth_prior = truth_prior + dmean.astype(np.longdouble)[None, :, :]
    truth = idr.path_gradient(c.X, Q, s, kernel, SIGMA2, paths.omega, paths.phase, W, v, dmean=dmean, dtype=np.longdouble)
    prior64 = np.abs(np.asarray(truth_prior, dtype=np.float64))
    bar_prior = np.transpose(idr.rffgrad_bar(Qt, s, paths.omega, paths.phase, W, SIGMA2), (2, 0, 1)) + 2. ** -52 * prior64
    bar = bar_prior + np.transpose(idr.kgrad_bar(Qt, Xt, s, kernel, SIGMA2, v), (2, 0, 1)) + 2. ** -52 * np.abs(np.asarray(truth, dtype=np.float64))
    return truth_prior, truth, bar_prior, bar


@pytest.mark.parametrize("kernel", [SE, M52])
def test_path_gradient_against_the_restatement_assembled_from_the_paths_own_fields(kernel):
    n, D, p, S = 300, 3, 64, 3
    c, s, ig = tg._iter(n, D, kernel, p)
    W, eps = ph.path_normals(n, S, F_SMALL, seed=3)
    paths = ig.sample_paths(S, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    Q = c.Xs
    g, pg = paths.gradient(Q), paths.prior_gradient(Q)
    assert g.shape == pg.shape == (S, Q.shape[0], D) and paths.converged.all()
    truth_prior, truth, bar_prior, bar = _path_bars(c, s, kernel, paths, Q, None)
    fp, fg = ih.fraction_of_bar(pg, truth_prior, bar_prior), ih.fraction_of_bar(g, truth, bar)
    print("n %d D %d %s: prior gradient at %.3g of its bar, path gradient at %.3g" % (n, D, kernel, fp, fg))
    assert fp <= 1. and fg <= 1.
    assert np.array_equal(pg, ig._native.rff_inputderiv(s, paths.omega, paths.phase, W, _amp(F_SMALL), Q))
    # a path is a function: the same bits whatever else is asked
    assert np.array_equal(paths.gradient(Q), g) and np.array_equal(paths.gradient(Q[5:6])[:, 0], g[:, 5])
    for mp in (1, 7, 64):
        assert np.array_equal(paths.gradient(Q, max_points=mp), g) and np.array_equal(paths.prior_gradient(Q, max_points=mp), pg), mp
    val, grad = paths.value_and_gradient(Q)
    assert np.array_equal(val, paths.evaluate(Q)) and np.array_equal(grad, g)
    ig.close()
    for call in (paths.gradient, paths.prior_gradient, paths.value_and_gradient):
        with pytest.raises(RuntimeError, match="the handle has been closed"):
            call(Q)


def test_gradient_of_path_s_is_the_gradient_of_the_single_draw_s():
    n, D, kernel, p, seed = 300, 3, M52, 64, 7
    c, s, ig = tg._iter(n, D, kernel, p)
    four = ig.sample_paths(4, n_features=F_SMALL, seed=seed).gradient(c.Xs)
    for d in range(4):
        one = ig.sample_paths(1, n_features=F_SMALL, seed=seed, first_draw=d).gradient(c.Xs)
        assert np.array_equal(one[0], four[d]), d
    assert not np.array_equal(four[0], four[1])
    ig.close()


def test_path_gradient_with_a_fixed_linear_mean():
    n, D, kernel, p, beta = th.LINEAR_MEAN
    c, (s,) = th.setup(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, np.r_[beta, c.thetas[0]], mean=LibGPGPU.PolyMeanFunc([[0, 1]]))
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    W, eps = ph.path_normals(n, 2, F_SMALL, seed=4)
    paths = ig.sample_paths(2, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    dmean = np.zeros(c.Xs.shape)
    dmean[:, 0] = beta[1]                                      # d (b0 + b1 x_0) / dx
    truth_prior, truth, bar_prior, bar = _path_bars(c, s, kernel, paths, c.Xs, dmean)
    fp, fg = ih.fraction_of_bar(paths.prior_gradient(c.Xs), truth_prior, bar_prior), ih.fraction_of_bar(paths.gradient(c.Xs), truth, bar)
    print("linear mean: prior gradient at %.3g of its bar, path gradient at %.3g" % (fp, fg))
    assert paths.converged.all() and fp <= 1. and fg <= 1.
    bare = ig._native.rff_inputderiv(s, paths.omega, paths.phase, W, _amp(F_SMALL), c.Xs)
    assert np.max(np.abs(paths.prior_gradient(c.Xs)[:, :, 0] - bare[:, :, 0])) > 1.       # the mean function's slope matters on these data
    assert np.array_equal(paths.prior_gradient(c.Xs)[:, :, 1:], bare[:, :, 1:])
    ig.close()


def test_vecchia_paths_have_the_gradient_of_the_view_on_the_same_handle():
    n, D, kernel, p = 300, 3, SE, 64
    c, s, ig = tg._iter(n, D, kernel, p)
    kw = dict(precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    want = ig.sample_paths(2, n_features=F_SMALL, seed=5).gradient(c.Xs)
    ig.close()
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, order=np.arange(n))
    got = vg.sample_paths(2, theta=c.thetas[0], n_features=F_SMALL, seed=5, **kw).gradient(c.Xs)
    assert np.array_equal(got, want)                           # the caller's order kept: the same data on the handle, the same bits
    vg.close()


# ---- the mean's derivative ------------------------------------------------------------------------------------------------------------------
def _deriv_bar(c, s, kernel, ig, y_resid, dense_deriv):
    """dimension_cases.BARS["deriv"] times the amplification, as test_gpu_iterative._check_against_dense forms its bars, plus the term for an
    inexact alpha: |d_d k*^T (alpha - A^-1 y)| <= |A^-1 d_d k*| |y - A alpha|, d_d k* the dense derivative of the cross covariance"""
    n, D = c.X.shape
    A, A80, cond, amp = tg._dense(n, D, kernel)
    Qt, Xt = ir.scaled(c.Xs, s), ir.scaled(c.X, s)
    gen = idr.generated(Qt, Xt, kernel, SIGMA2)
    rho = np.linalg.norm(y_resid - A @ ig.weights())
    rt, at = dc.BARS["deriv"]
    bar = amp * (at + rt * np.abs(dense_deriv))
    for d in range(D):
        dk = 2. * s[d] * gen * (Qt[:, d][:, None] - Xt[:, d][None, :])          # (m, n)
        bar[:, d] += np.linalg.norm(np.linalg.solve(A, dk.T), axis=0) * rho
    return bar


@pytest.mark.parametrize("n,D,kernel,p", th.PREDICT_SHAPES, ids=lambda v: str(v))
def test_predict_deriv_against_the_dense_predict(n, D, kernel, p):
    c, (s,) = th.setup(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    dense = gp.predict(c.Xs, unc=False, deriv=True)
    plain = ig.predict(c.Xs, unc=True)
    pr = ig.predict(c.Xs, unc=True, deriv=True)
    assert plain.deriv is None and pr.deriv.shape == dense.deriv.shape == (c.Xs.shape[0], D) and bool(pr.converged)
    for q in ("mean", "unc", "var_residual", "var_converged", "residual", "iterations"):
        assert np.array_equal(getattr(pr, q), getattr(plain, q)), q              # every other field keeps its bits
    frac = float(np.max(np.abs(pr.deriv - dense.deriv) / _deriv_bar(c, s, kernel, ig, c.T[0], dense.deriv)))
    print("n %d D %d %s p %d: d mean / dx at %.3g of its bar (largest entry %.3g)" % (n, D, kernel, p, frac, np.max(np.abs(dense.deriv))))
    assert frac <= 1.
    assert np.array_equal(pr.deriv, ig.matvec_inputderiv(ig.weights(), c.Xs))
    for mp in (1, 7):
        assert np.array_equal(ig.predict(c.Xs, deriv=True, max_points=mp).deriv, pr.deriv), mp
    assert np.array_equal(ig.predict(c.Xs[5:6], deriv=True).deriv[0], pr.deriv[5])
    ig.close()


def test_predict_deriv_with_a_fixed_linear_mean():
    n, D, kernel, p, beta = th.LINEAR_MEAN
    c, (s,) = th.setup(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, np.r_[beta, c.thetas[0]], mean=LibGPGPU.PolyMeanFunc([[0, 1]]))
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    dense = gp.predict(c.Xs, unc=False, deriv=True)
    pr = ig.predict(c.Xs, deriv=True)
    resid = c.T[0] - (beta[0] + beta[1] * c.X[:, 0])
    frac = float(np.max(np.abs(pr.deriv - dense.deriv) / _deriv_bar(c, s, kernel, ig, resid, dense.deriv)))
    print("linear mean: d mean / dx at %.3g of its bar" % frac)
    assert frac <= 1.
    kernel_part = ig.matvec_inputderiv(ig.weights(), c.Xs)
    assert np.array_equal(pr.deriv[:, 1:], kernel_part[:, 1:]) and np.max(np.abs(pr.deriv[:, 0] - kernel_part[:, 0] - beta[1])) <= 2. ** -50 * np.max(np.abs(pr.deriv))
    ig.close()


def test_multi_output_derivs_are_the_single_emulator_calls_and_the_vecchia_view_matches():
    n, D, kernel, p, E, nq = th.MULTI
    c, scales = th.setup(n, D, kernel, E=E)
    mo = M.MultiOutputGP_GPU(c.X[:tg.SUB], c.T[:, :tg.SUB], kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=c.nc, nugget_type="fixed"))
    mo.fit(c.thetas)
    ig = M.IterativeGP(mo, c.X, c.T, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    pr = ig.predict(c.Xs[:nq], deriv=True)
    assert pr.deriv.shape == (E, nq, D) and np.array_equal(ig.predict(c.Xs[:nq]).mean, pr.mean)
    kw = dict(precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    for e in range(E):
        ge = tg._gp(c.X[:tg.SUB], c.T[e, :tg.SUB], kernel, c.thetas[e])
        one = M.IterativeGP(ge, c.X, c.T[e], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        q = one.predict(c.Xs[:nq], deriv=True)
        assert np.array_equal(q.deriv, pr.deriv[e]) and np.array_equal(q.mean, pr.mean[e]), e
        V = th.matvec_input(n, 3)
        assert np.array_equal(one.matvec_inputderiv(V, c.Xs[:nq]), ig.matvec_inputderiv(V, c.Xs[:nq], emulator=e))
        one.close()
        if e == 0:
            vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, order=np.arange(n))
            got = vg.predict_exact(c.Xs[:nq], theta=c.thetas[0], deriv=True, **kw)
            assert np.array_equal(got.deriv, q.deriv) and np.array_equal(got.mean, q.mean)
            vg.close()
    assert not np.array_equal(pr.deriv[0], pr.deriv[1])
    ig.close()
