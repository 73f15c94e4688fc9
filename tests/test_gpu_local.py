"""Local approximate GP prediction on the MI355X (mogp_emulator_amd.LocalGP, csrc/kernels_local.hip) against the NumPy restatement
(local_restate.py), at the smallest shapes where the code can go another way: k below, at and above one wave of the best list (8, 50, 64,
126 = the tile's limit), a design of several staged tiles of 128 rows with a partial last one, k = N, every kernel, and the input dimension on
both sides of the other paths' thresholds and at both ends.

The neighbour lists and the radius are held to the restatement EXACTLY (the contract of include/mogp_hip.h makes the distance arithmetic
reproducible in NumPy); mean and variance are held, on the device's own lists, to dimension_cases.BARS times the amplification of every
query's own local matrix (1 throughout: test_local_host.py asserts cond <= 1.2e6 on these shapes, and that the restatement's own float64
error lies below the bars and above 0).  The measured figures are printed as fractions of their bars; DESIGN.md section 3 "Local
prediction" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import local_cases as lc
import local_restate as lr

pytestmark = pytest.mark.gpu

SUB = 64          # the emulator the hyperparameters come from is fitted on the first rows only: LocalGP must not look at its data


def _gp(X, t, kernel, theta, nugget=dc.NUGGET, mean=None):
    D = X.shape[1]
    gp = M.GaussianProcessGPU(X, t, mean=mean, kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=dc.n_corr(kernel, D), nugget_type="fixed"))
    gp.fit(theta)
    return gp


def _local(N, D, k, kernel):
    c, (s,) = lc.setup(N, D, kernel)
    gp = _gp(c.X[:SUB], c.T[0, :SUB], kernel, c.thetas[0])
    return c, s, M.LocalGP(gp, c.X, c.T[0], n_neighbours=k)


def _check_neighbours_and_values(N, D, k, kernel):
    c, s, lg = _local(N, D, k, kernel)
    ref = lc.reference(N, D, k, kernel)
    p = lg.predict(c.Xs, return_neighbours=True)
    lg.close()
    assert p.neighbours.shape == (lc.M, k) and p.neighbours.dtype == np.int64 and p.ok.all() and p.n_failed == 0
    assert np.array_equal(p.neighbours, ref["nbr"])
    assert np.array_equal(p.radius.view(np.int64), ref["radius"].view(np.int64))
    # values on the device's own lists (the restatement's, as just asserted)
    em, ev = lc.excess_rows("mean", p.mean, ref["mean"], ref["cond"]), lc.excess_rows("var", p.unc, ref["var"], ref["cond"])
    print("N %d D %d k %d %s: mean at %.3g of its bar, variance at %.3g (cond at most %.3g)" % (N, D, k, kernel, em, ev, ref["cond"].max()))
    assert em <= 1. and ev <= 1.


@pytest.mark.parametrize("kernel", lc.KERNELS)
@pytest.mark.parametrize("N,D,k", lc.SHAPES)
def test_neighbours_exactly_and_values_within_the_bars(N, D, k, kernel):
    _check_neighbours_and_values(N, D, k, kernel)


@pytest.mark.parametrize("kernel", lc.SWEEP_KERNELS)
@pytest.mark.parametrize("D", lc.D_ENDS_AND_EDGES)
def test_input_dimension(D, kernel):
    _check_neighbours_and_values(dc.N_TILES, D, lc.SWEEP_K, kernel)


@pytest.mark.parametrize("kernel", lc.SWEEP_KERNELS)
@pytest.mark.parametrize("N,D,k", lc.ODD_K)
def test_odd_neighbour_counts(N, D, k, kernel):
    _check_neighbours_and_values(N, D, k, kernel)


@pytest.mark.parametrize("kernel", lc.KERNELS)
def test_all_points_as_neighbours_is_the_dense_prediction(kernel):
    N, D, k = 126, 2, 126
    c, (s,) = lc.setup(N, D, kernel)
    ref = lc.reference(N, D, k, kernel)
    gp = _gp(c.X, c.T[0], kernel, c.thetas[0])
    dense = gp.predict(c.Xs, deriv=False)
    lg = M.LocalGP(gp, c.X, c.T[0], n_neighbours=k)
    p = lg.predict(c.Xs, return_neighbours=True)
    lg.close()
    assert p.ok.all()
    em, ev = lc.excess_rows("mean", p.mean, dense.mean, ref["cond"]), lc.excess_rows("var", p.unc, dense.unc, ref["cond"])
    print("k = N = 126 %s: local against dense predict: mean at %.3g of its bar, variance at %.3g" % (kernel, em, ev))
    assert em <= 1. and ev <= 1.
    for j in range(lc.M):
        assert np.array_equal(np.sort(p.neighbours[j]), np.arange(N))
        d = ref["r2"][j, p.neighbours[j]]
        assert np.all(np.diff(d) >= 0.) and d[-1] == p.radius[j]


def test_ties_go_to_the_lowest_index():
    lat = np.array([[i, j] for i in range(12) for j in range(12)], dtype=float)        # index 12 i + j
    t = np.sin(lat[:, 0]) + 0.1 * lat[:, 1]
    gp = _gp(lat[::7], t[::7], "SquaredExponential", np.zeros(3))                      # theta = 0: all scales 1
    for q, k, want in (((5.5, 5.5), 2, [65, 66]), ((5.5, 5.5), 3, [65, 66, 77]), ((5.5, 5.5), 4, [65, 66, 77, 78]), ((5, 5), 3, [65, 53, 64]),
                       ((5, 5), 5, [65, 53, 64, 66, 77])):
        p = M.predict_local(gp, lat, t, np.array([q], dtype=float), n_neighbours=k, return_neighbours=True)
        assert p.neighbours[0].tolist() == want, (q, k, p.neighbours[0])
        assert p.radius[0] == (0.5 if q[0] == 5.5 else (0. if k == 1 else 1.))
    # a repeated design point: the lower index first
    c, _ = lc.setup(300, 3, "Matern52")
    X = c.X.copy()
    X[7] = X[3]
    g2 = _gp(c.X[:SUB], c.T[0, :SUB], "Matern52", c.thetas[0])
    p = M.predict_local(g2, X, c.T[0], X[3:4], n_neighbours=4, return_neighbours=True)
    assert p.neighbours[0, :2].tolist() == [3, 7] and p.ok.all()


def _bits(p):
    return [p.mean.tobytes(), p.unc.tobytes(), p.ok.tobytes(), p.radius.tobytes(), p.neighbours.tobytes()]


def test_reproducibility_and_independence_of_the_grouping():
    N, D, k, kernel = 1000, 5, 64, "Matern52"
    c, s, lg = _local(N, D, k, kernel)
    first = lg.predict(c.Xs, return_neighbours=True)
    assert _bits(lg.predict(c.Xs, return_neighbours=True)) == _bits(first)
    for mp in (1, 7, lc.M):
        assert _bits(lg.predict(c.Xs, return_neighbours=True, max_points=mp)) == _bits(first), mp
    for j in (0, 5, 17, lc.M - 1):
        one = lg.predict(c.Xs[j:j + 1], return_neighbours=True)
        assert (one.mean[0].tobytes(), one.unc[0].tobytes(), one.radius[0].tobytes()) == (
            first.mean[j].tobytes(), first.unc[j].tobytes(), first.radius[j].tobytes()), j
        assert np.array_equal(one.neighbours[0], first.neighbours[j])
    # unc=False and include_nugget=False change nothing else
    bare = lg.predict(c.Xs, unc=False)
    assert bare.unc is None and bare.neighbours is None and bare.mean.tobytes() == first.mean.tobytes()
    nn = lg.predict(c.Xs, include_nugget=False)
    assert nn.mean.tobytes() == first.mean.tobytes() and np.all(nn.unc < first.unc)
    lg.close()


def _multi(c, thetas, kernel):
    mo = M.MultiOutputGP_GPU(c.X[:SUB], c.T[:, :SUB], kernel=kernel, nugget=dc.NUGGET, priors=GPPriors(n_corr=c.nc, nugget_type="fixed"))
    mo.fit(thetas)
    return mo


def test_multi_output_rows_are_the_single_emulator_calls():
    """E = 3 with the three theta of case(..., E=3): every row equals the single-emulator call bit for bit.  Those three theta differ by one
    constant added to every correlation parameter -- the same metric up to a factor -- so their neighbour LISTS coincide and only the radii
    differ; that every emulator searches in its own metric is therefore shown on a second model whose emulators carry the correlation
    parameters in rotated order: there the lists differ."""
    N, D, k, kernel = 300, 3, 50, "SquaredExponential"
    c, _ = lc.setup(N, D, kernel, E=3)
    rolled = np.stack([np.r_[np.roll(c.thetas[e][:D], e), c.thetas[e][D:]] for e in range(3)])
    for thetas, lists_differ in ((c.thetas, False), (rolled, True)):
        mo = _multi(c, thetas, kernel)
        lg = M.LocalGP(mo, c.X, c.T, n_neighbours=k)
        p = lg.predict(c.Xs, return_neighbours=True)
        lg.close()
        assert p.mean.shape == p.unc.shape == p.ok.shape == p.radius.shape == (3, lc.M) and p.neighbours.shape == (3, lc.M, k) and p.ok.all()
        for e in range(3):
            ge = _gp(c.X[:SUB], c.T[e, :SUB], kernel, thetas[e])
            one = M.predict_local(ge, c.X, c.T[e], c.Xs, n_neighbours=k, return_neighbours=True)
            assert _bits(one) == _bits(M.LocalPrediction(p.mean[e], p.unc[e], p.ok[e], p.radius[e], p.neighbours[e])), e
            nbr, radius, _ = lr.neighbours(c.X, c.Xs, lr.scales(thetas[e][:D], D, kernel), k)
            assert np.array_equal(p.neighbours[e], nbr) and np.array_equal(p.radius[e], radius)
        assert not np.array_equal(p.radius[0], p.radius[1]) and not np.array_equal(p.radius[1], p.radius[2])
        if lists_differ:
            assert not np.array_equal(p.neighbours[0], p.neighbours[1]) and not np.array_equal(p.neighbours[1], p.neighbours[2])


def test_fixed_linear_mean_is_subtracted_and_added_back():
    N, D, k, kernel = 300, 3, 50, "Matern52"
    c, (s,) = lc.setup(N, D, kernel)
    beta = np.array([0.7, -1.3])                              # c + c x[0], its coefficients fixed in theta
    gp = _gp(c.X[:SUB], c.T[0, :SUB], kernel, np.r_[beta, c.thetas[0]], mean=LibGPGPU.PolyMeanFunc([[0, 1]]))
    p = M.predict_local(gp, c.X, c.T[0], c.Xs, n_neighbours=k, return_neighbours=True)
    ref = lc.reference(N, D, k, kernel)
    assert np.array_equal(p.neighbours, ref["nbr"]) and p.ok.all()
    resid = c.T[0] - (beta[0] + beta[1] * c.X[:, 0])
    mean, var, ok, cond = lr.predict(c.X, resid, c.Xs, s, kernel, lc.SIGMA2, dc.NUGGET, p.neighbours)
    mean = mean + (beta[0] + beta[1] * c.Xs[:, 0])
    em, ev = lc.excess_rows("mean", p.mean, mean, cond), lc.excess_rows("var", p.unc, var, cond)
    print("linear mean: mean at %.3g of its bar, variance at %.3g" % (em, ev))
    assert em <= 1. and ev <= 1.
    assert np.max(np.abs(p.mean - ref["mean"])) > 1e-6        # the mean function matters on these data


def test_ok_flags_are_consistent_on_singular_local_matrices():
    """40 design points, each present three times, no nugget: every local matrix is exactly singular, and either decision of its
    factorisation is legitimate.  Whatever it decides, ok False <=> that row is NaN; with jitter every row is ok and within the bars."""
    D, k, kernel = 3, 30, "SquaredExponential"
    c, (s,) = lc.setup(300, D, kernel)
    X40, t40 = c.X[:40], c.T[0, :40]
    gp = _gp(X40, t40, kernel, c.thetas[0], nugget=0.)
    X, t = np.tile(X40, (3, 1)), np.tile(t40, 3)
    lg = M.LocalGP(gp, X, t, n_neighbours=k)
    p = lg.predict(c.Xs, return_neighbours=True)
    assert np.array_equal(p.ok, np.isfinite(p.mean)) and np.array_equal(p.ok, np.isfinite(p.unc))
    assert np.array_equal(~p.ok, np.isnan(p.mean)) and np.array_equal(~p.ok, np.isnan(p.unc))
    assert p.n_failed == int(np.sum(~p.ok))
    print("singular local matrices: %d of %d queries refused" % (p.n_failed, lc.M))
    jitter = 1e-4 * lc.SIGMA2
    pj = lg.predict(c.Xs, jitter=jitter, return_neighbours=True)
    lg.close()
    assert pj.ok.all() and pj.n_failed == 0 and np.array_equal(pj.neighbours, p.neighbours)
    mean, var, ok, cond = lr.predict(X, t, c.Xs, s, kernel, lc.SIGMA2, 0., pj.neighbours, jitter=jitter)
    assert ok.all()
    em, ev = lc.excess_rows("mean", pj.mean, mean, cond), lc.excess_rows("var", pj.unc, var, cond)
    print("    with jitter: mean at %.3g of its bar, variance at %.3g (cond at most %.3g)" % (em, ev, cond.max()))
    assert em <= 1. and ev <= 1.
