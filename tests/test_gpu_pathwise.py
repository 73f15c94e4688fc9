"""Pathwise posterior draws on the MI355X (mogp_emulator_amd.IterativeGP.sample_paths, csrc/kernels_rff.hip, csrc/engine_rff.hip) against the
NumPy restatement (pathwise_restate.py) and the dense GaussianProcessGPU.predict, at the smallest shapes where the code can go another way:
one, a partial and several tiles of 64 points and of 64 features, one and two MFMA blocks of 16 draws and a second pass of 32, both ends of
the input dimension, the design's rows and both query counts of dimension_cases, a squared-exponential and a Matern kernel.  Every design
here fits one block of 1024 rows: N = 1030 is in test_gpu_pathwise_large.py.

The product's cases, inputs and bar are those of test_pathwise_host.py, which shows on the CPU that float64 meets the bar and float32
frequencies miss it, and that the restatement's solver converges within 600 iterations on the right-hand sides solved here, where these
tests allow 1000.  Measured figures are printed as fractions of their bars; DESIGN.md section 3 "Pathwise posterior draws" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors
from mogp_emulator_amd.Sampling import philox_normals

import dimension_cases as dc
import iterative_restate as ir
import pathwise_restate as pw
import test_gpu_iterative as tg
import test_iterative_host as th
import test_pathwise_host as ph
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu

ETA = dc.NUGGET
F_SMALL = 64          # features of the tests that are not about the features: one tile


def _amp(F):
    return np.sqrt(2. * SIGMA2 / F)


_normals = ph.path_normals


# ---- the product ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mq,N,D,F,S,kernel", ph.PRODUCT_CASES, ids=lambda v: str(v))
def test_product_against_the_long_double_restatement(Mq, N, D, F, S, kernel):
    Pt, s, raw, c, omega, phase, W = ph.product_inputs(Mq, N, D, F, S, kernel)
    native = LibGPGPU.LocalGP_GPU(c.X, c.T[:1])
    got = native.rff(s, omega, phase, W, _amp(F), queries=raw).T
    native.close()
    assert got.shape == (Pt.shape[0], S)
    truth = pw.rff(Pt, omega, phase, W, SIGMA2, dtype=np.longdouble)
    frac = ph.fraction_of_bar(got, truth, pw.rff_bar(Pt, omega, phase, W, SIGMA2))
    print("M %d D %d F %d S %d %s: feature product at %.3g of its bar" % (Pt.shape[0], D, F, S, kernel, frac))
    assert frac <= 1.


def test_product_is_reproducible_and_its_columns_and_rows_are_independent():
    Mq, N, D, F, S, kernel = 130, 130, 3, 130, 33, "Matern52"
    Pt, s, raw, c, omega, phase, W = ph.product_inputs(Mq, N, D, F, S, kernel)
    native = LibGPGPU.LocalGP_GPU(c.X, c.T[:1])
    first = native.rff(s, omega, phase, W, _amp(F), queries=raw)
    assert first.shape == (S, Mq) and np.array_equal(native.rff(s, omega, phase, W, _amp(F), queries=raw), first)
    for j in (0, 7, 15, 16, 31, 32):
        assert np.array_equal(native.rff(s, omega, phase, W[j:j + 1], _amp(F), queries=raw)[0], first[j]), j
    assert np.array_equal(native.rff(s, omega, phase, W[5:22], _amp(F), queries=raw), first[5:22])
    for i in (0, 63, 64, 129):
        assert np.array_equal(native.rff(s, omega, phase, W, _amp(F), queries=raw[i:i + 1])[:, 0], first[:, i]), i
    for mp in (1, 64, 65):
        assert np.array_equal(native.rff(s, omega, phase, W, _amp(F), queries=raw, max_points=mp), first), mp
    # the design's rows: the same kernel on the rows the handle holds, in passes as well
    design = native.rff(s, omega, phase, W, _amp(F))
    assert design.shape == (S, N) and np.array_equal(native.rff(s, omega, phase, W, _amp(F), queries=c.X), design)
    for mp in (1, 64, 65):
        assert np.array_equal(native.rff(s, omega, phase, W, _amp(F), max_points=mp), design), mp
    native.close()


# ---- conditioning ------------------------------------------------------------------------------------------------------------------------
def conditioning_check(c, s, kernel, ig, y, paths, eps):
    """evaluate(X) + eta update + sqrt(eta) eps - y = A v - b, draw by draw: its norm over |b| against the reported residual plus what the
    two products' bars, the sums around them and the device's own dot allow; returns the largest (measured / allowed)"""
    n, D = c.X.shape
    F = paths.n_features
    A, A80, cond, amp = tg._dense(n, D, kernel)
    f = paths.evaluate(c.X)
    v, W = paths.update, paths.feature_normals
    assert f.shape == (paths.n_draws, n) and v.shape == (n, paths.n_draws)
    Xt = ir.scaled(c.X, s)
    g = pw.rff(Xt, paths.omega, paths.phase, W, SIGMA2)
    b = y[:, None] - g - np.sqrt(ETA) * eps.T
    back = (f + ETA * v.T + np.sqrt(ETA) * eps).T - y[:, None]
    K = A - ETA * np.eye(n)
    entry = (2. * pw.rff_bar(Xt, paths.omega, paths.phase, W, SIGMA2) + th.matvec_bar(np.abs(K), v, D)
             + 8. * 2. ** -52 * (np.abs(y)[:, None] + np.abs(g) + np.abs(K) @ np.abs(v) + ETA * np.abs(v) + np.sqrt(ETA) * np.abs(eps.T)))
    bn = np.linalg.norm(b, axis=0)
    measured = np.linalg.norm(back, axis=0) / bn
    allowed = paths.residual + np.linalg.norm(entry, axis=0) / bn + tg._residual_slack(A, b, v, D, paths.residual)
    print("n %d D %d %s F %d: |A v - b| / |b| from the paths %s, reported residuals %s, iterations %s"
          % (n, D, kernel, F, measured, paths.residual, paths.iterations.tolist()))
    return float(np.max(measured / allowed))


@pytest.mark.parametrize("n,D,kernel,p", th.PREDICT_SHAPES, ids=lambda v: str(v))
def test_paths_reproduce_the_data_up_to_the_reported_residual(n, D, kernel, p):
    c, s, ig = tg._iter(n, D, kernel, p)
    W, eps = _normals(n, 3, F_SMALL)
    paths = ig.sample_paths(3, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    assert paths.n_draws == 3 and paths.n_features == F_SMALL and paths.omega.shape == (F_SMALL, D) and paths.phase.shape == (F_SMALL,)
    assert np.array_equal(paths.feature_normals, W) and paths.precond_rank == p and paths.seed == 0 and paths.stream == 0x200
    assert paths.converged.all() and paths.ok.all() and paths.iterations.max() <= MAX_ITER and paths.iterations.min() >= 1
    worst = conditioning_check(c, s, kernel, ig, c.T[0], paths, eps)
    print("n %d D %d %s: conditioning identity at %.3g of what the residual and the products allow" % (n, D, kernel, worst))
    assert worst <= 1.
    # a path is a function: the same bits at the same point whatever else is asked, and no nugget is added
    q = paths.evaluate(c.Xs)
    assert q.shape == (3, c.Xs.shape[0]) and np.array_equal(paths(c.Xs), q) and np.array_equal(paths.evaluate(c.Xs[5:6])[:, 0], q[:, 5])
    for mp in (1, 7, 64):
        assert np.array_equal(paths.evaluate(c.Xs, max_points=mp), q), mp
    assert np.array_equal(paths.prior(c.Xs), ig._native.rff(s, paths.omega, paths.phase, W, _amp(F_SMALL), queries=c.Xs))
    again = ig.sample_paths(3, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    assert np.array_equal(again.update, paths.update) and np.array_equal(again.residual, paths.residual)
    ig.close()
    with pytest.raises(RuntimeError, match="PosteriorPaths.evaluate: the handle has been closed"):
        paths.evaluate(c.Xs)


@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_antithetic_pair_averages_to_the_posterior_mean(kernel):
    n, D, p = 300, 3, 64
    c, (s,) = th.setup(n, D, kernel)
    A, A80, cond, amp = tg._dense(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, c.thetas[0])
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    W, eps = _normals(n, 1, F_SMALL, seed=2)
    paths = ig.sample_paths(2, n_features=F_SMALL, feature_normals=np.vstack([W, -W]), noise_normals=np.vstack([eps, -eps]))
    f = paths.evaluate(c.Xs)
    ig.close()
    dense = gp.predict(c.Xs, deriv=False)
    got = 0.5 * (f[0] + f[1])
    vbar = 0.5 * (paths.update[:, 0] + paths.update[:, 1])
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    wn = np.linalg.norm(np.linalg.solve(A, ks), axis=0)
    rho = np.linalg.norm(c.T[0] - A @ vbar)                    # exact algebra for an inexact solve, as test_predict_against_the_dense_predict
    rt, at = dc.BARS["mean"]
    frac = float(np.max(np.abs(got - dense.mean) / (amp * (at + rt * np.abs(dense.mean)) + wn * rho)))
    print("n %d D %d %s: antithetic average at %.3g of the mean's bar; the two paths differ by up to %.3g" % (n, D, kernel, frac, np.max(np.abs(f[0] - f[1]))))
    assert paths.converged.all() and frac <= 1.
    assert np.max(np.abs(f[0] - f[1])) > 1e-3                  # the pair is a pair of different functions


def _dense_bar(c, s, kernel, y, paths, W, eps, Q):
    """(truth (S, m) long double, bar (S, m)): the restatement's own float64 gap to its long-double form (the largest entry of the draw),
    scaled by dimension_cases.amplification as test_gpu_iterative._check_against_dense scales its bars, plus that function's term for a solve
    that is not exact: |k*^T (v - A^-1 b)| <= |A^-1 k*| |b - A v|"""
    n, D = c.X.shape
    A, A80, cond, amp = tg._dense(n, D, kernel)
    truth, _, b80 = pw.paths(c.X, y, Q, s, kernel, SIGMA2, ETA, paths.omega, paths.phase, W, eps, dtype=np.longdouble)
    f64 = pw.paths(c.X, y, Q, s, kernel, SIGMA2, ETA, paths.omega, paths.phase, W, eps)[0]
    gap = np.max(np.abs(np.asarray(f64.astype(np.longdouble) - truth, dtype=np.float64)), axis=1)
    wn = np.linalg.norm(np.linalg.solve(A, ir.covariance(c.X, Q, s, kernel, SIGMA2)), axis=0)
    bn = np.linalg.norm(np.asarray(b80, dtype=np.float64), axis=0)
    return truth, amp * gap[:, None] + wn[None, :] * (paths.residual * bn)[:, None], gap, wn


@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_paths_against_the_restatements_dense_solve(kernel):
    n, D, p, S = 300, 3, 64, 3
    c, s, ig = tg._iter(n, D, kernel, p)
    W, eps = _normals(n, S, F_SMALL, seed=3)
    paths = ig.sample_paths(S, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    f = paths.evaluate(c.Xs)
    ig.close()
    truth, bar, gap, wn = _dense_bar(c, s, kernel, c.T[0], paths, W, eps, c.Xs)
    frac = ph.fraction_of_bar(f, truth, bar)
    print("n %d D %d %s: paths at %.3g of their bar (float64 restatement's gap %s, residuals %s)" % (n, D, kernel, frac, gap, paths.residual))
    assert paths.converged.all() and frac <= 1.


def test_default_generator_is_the_restated_one_and_first_draw_splits_a_call():
    n, D, kernel, p, S, seed = 300, 3, "Matern52", 64, 4, 7
    c, s, ig = tg._iter(n, D, kernel, p)
    paths = ig.sample_paths(S, n_features=F_SMALL, seed=seed)
    sub = 0x200
    omega, phase = pw.features(seed, sub, F_SMALL, D, kernel)
    W, eps = philox_normals(seed, sub + 3, S, F_SMALL), philox_normals(seed, sub + 4, S, n)
    assert np.array_equal(paths.omega, omega) and np.array_equal(paths.phase, phase) and paths.seed == seed and paths.stream == sub
    dis = float(np.max(np.abs(paths.feature_normals - W)))
    print("device normals of the weights vs philox_normals %.3g (bar 1e-13)" % dis)
    assert dis <= 1e-13                                        # what test_gpu_sample.py allows the device's normals
    f = paths.evaluate(c.Xs)
    # the restatement on the weights the device used and the restated noise; the device's noise may differ from it by 1e-13 per normal
    truth, bar, gap, wn = _dense_bar(c, s, kernel, c.T[0], paths, paths.feature_normals, eps, c.Xs)
    bar = bar + wn[None, :] * np.sqrt(ETA) * 1e-13 * np.sqrt(n)
    frac = ph.fraction_of_bar(f, truth, bar)
    print("default generator: paths at %.3g of their bar" % frac)
    assert paths.converged.all() and frac <= 1.
    # bit for bit: a repeated call, and the call split in two
    again = ig.sample_paths(S, n_features=F_SMALL, seed=seed)
    a, b = ig.sample_paths(2, n_features=F_SMALL, seed=seed), ig.sample_paths(2, n_features=F_SMALL, seed=seed, first_draw=2)
    for q in ("update", "feature_normals", "residual", "iterations", "converged"):
        assert np.array_equal(getattr(again, q), getattr(paths, q)), q
        assert np.array_equal(np.concatenate([getattr(a, q), getattr(b, q)], axis=-1 if q == "update" else 0), getattr(paths, q)), q
    assert np.array_equal(np.vstack([a.evaluate(c.Xs), b.evaluate(c.Xs)]), f)
    other = ig.sample_paths(1, n_features=F_SMALL, seed=seed + 1)
    assert not np.array_equal(other.update[:, 0], paths.update[:, 0])
    ig.close()


# ---- the other entry points ---------------------------------------------------------------------------------------------------------------
def test_an_emulator_of_a_model_is_the_single_emulator_call_at_its_stream():
    n, D, kernel, p, E, nq = th.MULTI
    c, scales = th.setup(n, D, kernel, E=E)
    mo = M.MultiOutputGP_GPU(c.X[:tg.SUB], c.T[:, :tg.SUB], kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=c.nc, nugget_type="fixed"))
    mo.fit(c.thetas)
    ig = M.IterativeGP(mo, c.X, c.T, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    got = ig.sample_paths(2, emulator=1, n_features=F_SMALL, seed=3)
    ge = tg._gp(c.X[:tg.SUB], c.T[1, :tg.SUB], kernel, c.thetas[1])
    one = M.IterativeGP(ge, c.X, c.T[1], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    want = one.sample_paths(2, n_features=F_SMALL, seed=3, stream=0x200 + 8)
    assert got.stream == want.stream == 0x208 and got.emulator == 1 and got.converged.all()
    for q in ("omega", "phase", "feature_normals", "update", "residual", "iterations"):
        assert np.array_equal(getattr(got, q), getattr(want, q)), q
    assert np.array_equal(got.evaluate(c.Xs[:nq]), want.evaluate(c.Xs[:nq]))
    zero = ig.sample_paths(2, emulator=0, n_features=F_SMALL, seed=3)
    assert not np.array_equal(zero.omega, got.omega) and not np.array_equal(zero.update, got.update)
    with pytest.raises(ValueError, match="IterativeGP.sample_paths: emulator must be between 0 and 2"):
        ig.sample_paths(2, emulator=3)
    one.close()
    ig.close()


def test_vecchia_sample_paths_is_the_view_on_the_same_handle():
    n, D, kernel, p = 300, 3, "SquaredExponential", 64
    c, s, ig = tg._iter(n, D, kernel, p)
    kw = dict(precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    want = ig.sample_paths(2, n_features=F_SMALL, seed=5)
    wq = want.evaluate(c.Xs)
    ig.close()
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=10, nugget=dc.NUGGET, order=np.arange(n))
    with pytest.raises(RuntimeError, match="VecchiaGP.sample_paths: fit has not been called and no theta was given"):
        vg.sample_paths(2)
    got = vg.sample_paths(2, theta=c.thetas[0], n_features=F_SMALL, seed=5, **kw)
    view = vg.exact_view(c.thetas[0], **kw).sample_paths(2, n_features=F_SMALL, seed=5)
    for q in ("omega", "phase", "feature_normals", "update", "residual", "iterations", "converged"):
        assert np.array_equal(getattr(got, q), getattr(view, q)), q
        assert np.array_equal(getattr(got, q), getattr(want, q)), q          # the caller's order kept: the same data on the handle, the same bits
    assert np.array_equal(got.evaluate(c.Xs), view.evaluate(c.Xs)) and np.array_equal(got.evaluate(c.Xs), wq)
    vg.close()


def test_fixed_linear_mean_is_subtracted_and_added_back():
    n, D, kernel, p, beta = th.LINEAR_MEAN
    c, (s,) = th.setup(n, D, kernel)
    gp = tg._gp(c.X, c.T[0], kernel, np.r_[beta, c.thetas[0]], mean=LibGPGPU.PolyMeanFunc([[0, 1]]))
    ig = M.IterativeGP(gp, c.X, c.T[0], precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    W, eps = _normals(n, 2, F_SMALL, seed=4)
    paths = ig.sample_paths(2, n_features=F_SMALL, feature_normals=W, noise_normals=eps)
    mean_x, mean_q = beta[0] + beta[1] * c.X[:, 0], beta[0] + beta[1] * c.Xs[:, 0]

    class _Shifted(object):                                    # the paths of the residual: what the identity is stated for
        def __init__(self, inner):
            self.__dict__.update(inner.__dict__)
            self.evaluate = lambda X: inner.evaluate(X) - mean_x[None, :]
    worst = conditioning_check(c, s, kernel, ig, c.T[0] - mean_x, _Shifted(paths), eps)
    assert paths.converged.all() and worst <= 1.
    g = ig._native.rff(s, paths.omega, paths.phase, W, _amp(F_SMALL), queries=c.Xs)
    assert np.max(np.abs(paths.prior(c.Xs) - g - mean_q[None, :])) <= 4. * 2. ** -52 * np.max(np.abs(g) + np.abs(mean_q))
    assert np.max(np.abs(mean_q)) > 1e-2                       # the mean function matters on these data
    ig.close()


def test_a_path_whose_solve_does_not_converge_is_reported_not_raised():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, s, ig = tg._iter(n, D, kernel, p, max_iter=2)
    paths = ig.sample_paths(3, n_features=F_SMALL, seed=1)
    f = paths.evaluate(c.Xs)
    ig.close()
    print("max_iter 2: residual %s" % paths.residual)
    assert not paths.converged.any() and not paths.ok.any() and np.all(paths.iterations == 2)
    assert np.all(np.isfinite(paths.update)) and np.all(np.isfinite(f)) and np.all(paths.residual > RTOL)
