"""The Vecchia likelihood on the MI355X (mogp_emulator_amd.VecchiaGP, csrc/kernels_local.hip) against the NumPy restatement
(vecchia_restate.py), at the smallest shapes where the code can go another way: k below, at and above one wave of the best list, the tile's
limit k = 126 (127 rows of the matrix proper and the target row), designs of several staged tiles with a partial last one, the first k points
with their shorter lists (k_t = 0 .. k inside one launch), every kernel, the nugget fitted and fixed, three orders, and the input dimension on
both sides of the other paths' thresholds and at both ends.

The neighbour lists are held to the restatement EXACTLY; on the device's own lists every term is held to dimension_cases.BARS["logpost"]
times the amplification of its own local matrix (1 throughout: test_vecchia_host.py asserts cond <= 1e7 on these shapes, and that the
restatement's own float64 error lies below the bars and above 0), and the gradient to BARS["grad"].  The measured figures are printed as
fractions of their bars; DESIGN.md section 3 "Vecchia fit" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd.Priors import GPPriors

import dimension_cases as dc
import local_restate as lr
import vecchia_cases as vc
import vecchia_restate as vr

pytestmark = pytest.mark.gpu


def _vecchia(N, D, k, kernel, fit, order_name, **kw):
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, fit)
    order = vc.order_of(order_name, N)
    vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=k, nugget="fit" if fit else dc.NUGGET, order=order, **kw)
    return c, theta, order, vg


# ---- neighbours ------------------------------------------------------------------------------------------------------------------------
def _check_neighbours(N, D, k, order_name):
    kernel = "SquaredExponential"
    c, theta, order, vg = _vecchia(N, D, k, kernel, False, order_name)
    vg.set_neighbours(theta=theta)
    got = vg.neighbours
    vg.close()
    _, pos, want = vc.neighbours(N, D, k, kernel, order_name)
    assert got.shape == (N, k) and got.dtype == np.int64
    assert np.array_equal(got, want)
    # the first k positions are padded: position p has p neighbours
    for p in range(min(k, N)):
        assert np.count_nonzero(got[order[p]] >= 0) == p and np.all(got[order[p]][p:] == -1)


@pytest.mark.parametrize("order_name", vc.ORDERS)
@pytest.mark.parametrize("N,D,k", vc.NEIGHBOUR_SHAPES)
def test_ordered_neighbours_exactly(N, D, k, order_name):
    _check_neighbours(N, D, k, order_name)


@pytest.mark.parametrize("order_name", vc.ORDERS)
@pytest.mark.parametrize("D", vc.NEIGHBOUR_SWEEP_D)
def test_ordered_neighbours_input_dimension(D, order_name):
    _check_neighbours(dc.N_TILES, D, 16, order_name)


def test_ties_go_to_the_lowest_position():
    lat = np.array([[i, j] for i in range(12) for j in range(12)], dtype=float)        # index 12 i + j
    t = np.sin(lat[:, 0]) + 0.1 * lat[:, 1]
    vg = M.VecchiaGP(lat, t, n_neighbours=4, order=np.arange(144))
    vg.set_neighbours()                                                                # all scales 1: small integers, exact
    got = vg.neighbours
    vg.close()
    assert np.array_equal(got, vr.ordered_neighbours(lat, np.ones(2), 4))
    assert got[65].tolist() == [53, 64, 52, 54] and got[13].tolist() == [1, 12, 0, 2] and got[1].tolist() == [0, -1, -1, -1]
    # reversed: the lowest POSITION is the highest index
    rev = np.arange(144)[::-1].copy()
    vg = M.VecchiaGP(lat, t, n_neighbours=4, order=rev)
    vg.set_neighbours()
    got = vg.neighbours
    vg.close()
    assert got[65].tolist() == [77, 66, 78, 76]
    # a repeated design row, three times: the lower position first
    c, theta, s, _, _ = vc.setup(300, 3, "Matern52", False)
    X = c.X.copy()
    X[7] = X[3]
    X[9] = X[3]
    vg = M.VecchiaGP(X, c.T[0], kernel="Matern52", n_neighbours=4, nugget=dc.NUGGET, order=np.arange(300))
    vg.set_neighbours(theta=theta)
    got = vg.neighbours
    vg.close()
    assert got[9, :2].tolist() == [3, 7] and got[7, 0] == 3 and got[20, :3].tolist() == vr.ordered_neighbours(X, s, 4)[20, :3].tolist()
    assert np.array_equal(got, vr.ordered_neighbours(X, s, 4))


# ---- terms, value, gradient ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,k,kernel,fit", vc.VALUE_CASES, ids=lambda v: str(v))
def test_terms_and_gradient_within_the_bars(N, D, k, kernel, fit):
    c, theta, order, vg = _vecchia(N, D, k, kernel, fit, "random")
    ref = vc.reference(N, D, k, kernel, fit)
    vg.set_neighbours(theta=theta)
    assert np.array_equal(vc.to_positions(vg.neighbours, order), ref["nbr"])           # the device's own lists are the restatement's
    ll = vg.loglik(theta, grad=True, return_terms=True)
    vg.close()
    assert ll.ok.all() and ll.n_failed == 0 and ll.terms.shape == (N,) and ll.grad.shape == (len(theta),)
    et = vc.excess_rows("logpost", ll.terms[order], ref["terms"], ref["cond"])
    amp = max(1., float(ref["cond"].max()) * 1e-7)
    want_v, want_g = ref["terms"].sum(), ref["grad"].sum(axis=0)
    ev = dc.excess("logpost", np.array([ll.value]), np.array([want_v]), amp)
    eg = dc.excess("grad", ll.grad, want_g, amp, max(1., float(np.max(np.abs(ll.grad)))))
    print("N %d D %d k %d %s nugget %s: terms at %.3g of their bar, value at %.3g, gradient at %.3g (cond at most %.3g)"
          % (N, D, k, kernel, "fit" if fit else "fixed", et, ev, eg, ref["cond"].max()))
    assert amp == 1.
    assert et <= 1. and ev <= 1. and eg <= 1.


@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_all_predecessors_as_neighbours_is_the_exact_likelihood(kernel):
    N, D, k = vc.LIMIT
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, True)
    want_v, want_g = vr.dense_loglik(c.X, c.T[0], s, kernel, sigma2, nugget, grad=True)
    r2 = lr.scaled_r2(c.X, c.X, s)
    cond, amp = dc.amplification(sigma2 * lr.kernel_of_r2(r2, kernel) + nugget * np.eye(N))
    for order_name in ("identity", "random"):
        order = vc.order_of(order_name, N)
        vg = M.VecchiaGP(c.X, c.T[0], kernel=kernel, n_neighbours=k, order=order)
        vg.set_neighbours(theta=theta)
        ll = vg.loglik(theta, grad=True)
        vg.close()
        ev = dc.excess("logpost", np.array([ll.value]), np.array([want_v]), amp)
        eg = dc.excess("grad", ll.grad, want_g, amp, max(1., float(np.max(np.abs(ll.grad)))))
        print("k = N - 1 = 126 %s, %s order: value at %.3g of its bar against the dense log-likelihood, gradient at %.3g (cond %.3g)"
              % (kernel, order_name, ev, eg, cond))
        assert ll.ok.all() and ev <= 1. and eg <= 1.


def test_every_length_of_list_inside_one_launch():
    """k = 126 at N = 130: positions 0 .. 125 have 0 .. 125 neighbours, the rest 126"""
    N, D, k, kernel = 130, 3, 126, "Matern52"
    c, theta, order, vg = _vecchia(N, D, k, kernel, True, "random")
    _, _, s, sigma2, nugget = vc.setup(N, D, kernel, True)
    vg.set_neighbours(theta=theta)
    pos = vc.to_positions(vg.neighbours, order)
    ll = vg.loglik(theta, return_terms=True)
    vg.close()
    rows = [0, 1, 2, 125, 126, 129]
    terms, _, ok, cond = vr.terms(c.X[order], c.T[0][order], s, kernel, sigma2, nugget, pos, rows=rows)
    for p in rows:
        assert np.count_nonzero(pos[p] >= 0) == min(p, k)
        e = dc.excess("logpost", ll.terms[order[p]:order[p] + 1], terms[p:p + 1], max(1., cond[p] * 1e-7))
        print("position %d (%d neighbours): term at %.3g of its bar" % (p, min(p, k), e))
        assert ok[p] and e <= 1.
    y0 = c.T[0][order[0]]
    closed = -0.5 * np.log(sigma2 + nugget) - 0.5 * y0 * y0 / (sigma2 + nugget) - 0.5 * np.log(2. * np.pi)
    assert dc.excess("logpost", ll.terms[order[0]:order[0] + 1], np.array([closed])) <= 1.


def test_the_same_bits_whatever_the_launches():
    N, D, k, kernel = 300, 3, 50, "Matern52"
    c, theta, order, vg = _vecchia(N, D, k, kernel, True, "random")
    vg.set_neighbours(theta=theta)
    first = vg.loglik(theta, grad=True, return_terms=True)

    def bits(ll):
        return (np.float64(ll.value).tobytes(), ll.grad.tobytes())
    again = vg.loglik(theta, grad=True, return_terms=True)
    assert bits(again) == bits(first) and again.terms.tobytes() == first.terms.tobytes()
    for mp in (1, 7, N):
        ll = vg.loglik(theta, grad=True, return_terms=True, max_points=mp)
        assert bits(ll) == bits(first) and ll.terms.tobytes() == first.terms.tobytes(), mp
    bare = vg.loglik(theta, grad=True)
    assert bare.terms is None and bits(bare) == bits(first)
    for mp in (0, 7):
        v = vg.loglik(theta, max_points=mp)
        assert v.grad is None and np.float64(v.value).tobytes() == np.float64(first.value).tobytes(), mp
    # a second search gives the same lists, and the likelihood on them the same bits
    nbr = vg.neighbours
    vg.set_neighbours(theta=theta)
    assert np.array_equal(vg.neighbours, nbr) and bits(vg.loglik(theta, grad=True)) == bits(first)
    vg.close()


def test_failure_is_local():
    """40 points, each present three times, a fixed nugget of 0: the matrices of the repeated points are exactly singular"""
    D, k, kernel = 3, 30, "SquaredExponential"
    c, theta, s, sigma2, _ = vc.setup(300, D, kernel, False)
    X, t = np.tile(c.X[:40], (3, 1)), np.tile(c.T[0, :40], 3)
    vg = M.VecchiaGP(X, t, kernel=kernel, n_neighbours=k, nugget=0., order=np.arange(120))
    vg.set_neighbours(theta=theta)
    ll = vg.loglik(theta, grad=True, return_terms=True)
    assert np.array_equal(~ll.ok, np.isnan(ll.terms)) and ll.n_failed == int(np.sum(~ll.ok))
    print("singular local matrices: %d of 120 points refused" % ll.n_failed)
    assert ll.n_failed > 0 and ll.value == -np.inf and np.all(np.isnan(ll.grad))
    jitter = 1e-4 * sigma2
    lj = vg.loglik(theta, grad=True, return_terms=True, jitter=jitter)
    pos = vc.to_positions(vg.neighbours, np.arange(120))
    vg.close()
    assert lj.ok.all() and lj.n_failed == 0 and np.isfinite(lj.value)
    terms, g, ok, cond = vr.terms(X, t, s, kernel, sigma2, 0., pos, jitter=jitter, grad=True, fit_nugget=False)
    assert ok.all()
    et = vc.excess_rows("logpost", lj.terms, terms, cond)
    amp = max(1., float(cond.max()) * 1e-7)
    eg = dc.excess("grad", lj.grad, g.sum(axis=0), amp, max(1., float(np.max(np.abs(lj.grad)))))
    print("    with jitter: terms at %.3g of their bar, gradient at %.3g (cond at most %.3g)" % (et, eg, cond.max()))
    assert et <= 1. and eg <= 1.


# ---- fit and predict -------------------------------------------------------------------------------------------------------------------------
FIT = dict(N=600, D=2, k=20, kernel="SquaredExponential")


def _fit_problem():
    N, D, kernel = FIT["N"], FIT["D"], FIT["kernel"]
    c = dc.case(N, D, kernel, fit=True)
    truth = c.thetas[0]
    s, sigma2, nugget = vr.unpack(truth, D, kernel, "fit")
    return c.X, vr.draw(c.X, s, kernel, sigma2, nugget, seed=1), truth, c.Xs


@pytest.mark.parametrize("refresh", [0, 2])
def test_fit_reaches_a_stationary_point_of_the_likelihood_on_its_final_lists(refresh):
    X, y, truth, _ = _fit_problem()
    N, D, k, kernel = FIT["N"], FIT["D"], FIT["k"], FIT["kernel"]
    vg = M.VecchiaGP(X, y, kernel=kernel, n_neighbours=k, rng=3)
    fit = vg.fit(refresh=refresh)
    order, nbr = vg.order, vg.neighbours
    at_start = fit.tries[0]["start_value"]
    vg.close()
    assert len(fit.tries) == 1 and fit.n_refreshes == refresh and fit.converged and fit.n_evaluations >= 2 * (refresh + 1)
    assert np.isfinite(fit.value) and fit.value >= at_start
    v, g = vr.loglik_theta(X[order], y[order], fit.theta, kernel, "fit", vc.to_positions(nbr, order), grad=True)
    gtol = 1e-5 * N                              # the projected-gradient rule fit used (no bounds: the gradient itself)
    print("refresh %d: %d evaluations, value %.6f (start %.3f), restated %.6f, largest gradient entry %.3g (rule %.3g), theta - truth %s"
          % (refresh, fit.n_evaluations, fit.value, at_start, v, np.max(np.abs(g)), gtol, np.array2string(fit.theta - truth, precision=3)))
    assert dc.excess("logpost", np.array([fit.value]), np.array([v])) <= 1.
    assert np.max(np.abs(g)) <= 10. * gtol


def test_fit_keeps_the_best_try_and_the_lists_its_value_was_computed_on():
    c, theta, order, vg = _vecchia(300, 3, 8, "Matern52", True, "random")
    fit = vg.fit(theta0=theta, n_tries=3, refresh=1, rng=5, maxiter=6)
    assert len(fit.tries) == 3 and fit.value == max(t["value"] for t in fit.tries)
    assert all(t["n_refreshes"] == 1 and t["n_evaluations"] >= 2 for t in fit.tries)
    assert not np.array_equal(fit.tries[1]["theta0"], fit.tries[0]["theta0"]) and np.array_equal(fit.tries[0]["theta0"], theta)
    again = vg.loglik(fit.theta, grad=True)
    vg.close()
    assert np.float64(again.value).tobytes() == np.float64(fit.value).tobytes() and again.grad.tobytes() == fit.grad.tobytes()


def test_predict_is_local_prediction_at_the_fitted_theta():
    X, y, truth, Q = _fit_problem()
    N, D, k, kernel = FIT["N"], FIT["D"], FIT["k"], FIT["kernel"]
    vg = M.VecchiaGP(X, y, kernel=kernel, n_neighbours=k, rng=3)
    fit = vg.fit(refresh=1, maxiter=15)
    p = vg.predict(Q, return_neighbours=True)
    p50 = vg.predict(Q, n_neighbours=50, return_neighbours=True)
    vg.close()
    gp = M.GaussianProcessGPU(X[:64], y[:64], kernel=kernel, nugget=float(np.exp(fit.theta[-1])), priors=GPPriors(n_corr=D, nugget_type="fixed"))
    gp.fit(fit.theta[:-1])
    for got, kk in ((p, k), (p50, 50)):
        want = M.predict_local(gp, X, y, Q, n_neighbours=kk, return_neighbours=True)
        assert got.ok.all() and np.array_equal(got.neighbours, want.neighbours)
        assert [got.mean.tobytes(), got.unc.tobytes(), got.ok.tobytes(), got.radius.tobytes()] == [
            want.mean.tobytes(), want.unc.tobytes(), want.ok.tobytes(), want.radius.tobytes()], kk
