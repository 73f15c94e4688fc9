"""Host-side checks of the Vecchia likelihood (mogp_emulator_amd.VecchiaGP): the NumPy restatement (vecchia_restate.py) against central
differences of its own value, against the dense log-likelihood at k = N - 1 and against the closed form of the first term; the restatement in
float64 against itself in long double on the shapes of the GPU tests -- which proves that the bars the device is held to are not vacuous: the
float64 error lies below them and above 0, and every local matrix is conditioned well enough for an amplification of 1; vecchia_plan
(csrc/predict_plan.h) against a hand-worked table through a sanitised stand-alone program; the exports; and the argument refusals, which
come before any device call."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

VG = importlib.import_module("mogp_emulator_amd.Vecchia")

import dimension_cases as dc
import local_restate as lr
import vecchia_cases as vc
import vecchia_restate as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vecchia_plan_matches_the_hand_worked_table(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "vecchia_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "vecchia_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok 12 rows"


def test_exports():
    assert M.VecchiaGP is VG.VecchiaGP and M.VecchiaLogLik is VG.VecchiaLogLik and M.VecchiaFit is VG.VecchiaFit
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        for name in ("mogp_local_vecchia_neighbours", "mogp_local_vecchia_loglik"):
            assert name in _capi.SIGNATURES
        assert hasattr(LibGPGPU.LocalGP_GPU, "vecchia_neighbours") and hasattr(LibGPGPU.LocalGP_GPU, "vecchia_loglik")
    header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "mogp_local_vecchia_neighbours(" in header and "mogp_local_vecchia_loglik(" in header


# ---- the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [True, False], ids=["nugget fit", "nugget fixed"])
@pytest.mark.parametrize("kernel", vc.KERNELS)
def test_restated_gradient_is_the_derivative_of_the_restated_value(kernel, fit):
    N, D, k = 60, 3, 10
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, fit)
    order = vc.order_of("random", N)
    X, y = c.X[order], c.T[0][order]
    nbr = vr.ordered_neighbours(X, s, k)
    mode = "fit" if fit else dc.NUGGET
    v, g = vr.loglik_theta(X, y, theta, kernel, mode, nbr, grad=True)
    assert g.shape == (vr.n_params(D, kernel, fit),)
    h = 1e-5
    for p in range(len(theta)):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        num = (vr.loglik_theta(X, y, tp, kernel, mode, nbr)[0] - vr.loglik_theta(X, y, tm, kernel, mode, nbr)[0]) / (2. * h)
        # central differences: truncation h^2 |f'''| / 6 and rounding eps |f| / h, both far below 1e-5 of the scale
        assert abs(num - g[p]) <= 1e-5 * max(1., abs(g[p])), (p, num, g[p])


@pytest.mark.parametrize("order_name", vc.ORDERS)
@pytest.mark.parametrize("kernel", ["SquaredExponential", "UniformMat52"])
def test_all_predecessors_as_neighbours_is_the_dense_log_likelihood(kernel, order_name):
    N, D = 40, 2
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, True)
    order = vc.order_of(order_name, N)
    X, y = c.X[order], c.T[0][order]
    nbr = vr.ordered_neighbours(X, s, N - 1)
    assert all(np.array_equal(np.sort(nbr[t][:t]), np.arange(t)) and np.all(nbr[t][t:] == -1) for t in range(N))
    v, g = vr.loglik(X, y, s, kernel, sigma2, nugget, nbr, grad=True)
    dv, dg = vr.dense_loglik(c.X, c.T[0], s, kernel, sigma2, nugget, grad=True)         # the caller's order: the dense value has none
    assert abs(v - dv) <= 1e-10 * abs(dv) and np.all(np.abs(g - dg) <= 1e-8 * np.maximum(1., np.abs(dg)))


def test_the_first_term_in_closed_form():
    c, theta, s, sigma2, nugget = vc.setup(130, 3, "Matern52", True)
    nbr = vr.ordered_neighbours(c.X, s, 8)
    terms, _, ok, _ = vr.terms(c.X, c.T[0], s, "Matern52", sigma2, nugget, nbr, rows=[0])
    y0, v = c.T[0][0], sigma2 + nugget
    assert ok[0] and np.all(nbr[0] == -1)
    assert abs(terms[0] - (-0.5 * np.log(v) - 0.5 * y0 * y0 / v - 0.5 * np.log(2. * np.pi))) <= 1e-14


def test_restatement_reproduces_the_lattice_ties():
    lat = np.array([[i, j] for i in range(12) for j in range(12)], dtype=float)
    nbr = vr.ordered_neighbours(lat, np.ones(2), 4)
    assert nbr[65].tolist() == [53, 64, 52, 54] and nbr[13].tolist() == [1, 12, 0, 2] and nbr[1].tolist() == [0, -1, -1, -1]
    rev = np.arange(144)[::-1].copy()
    assert vc.to_caller(vr.ordered_neighbours(lat[rev], np.ones(2), 4), rev)[65].tolist() == [77, 66, 78, 76]
    pos = vr.ordered_neighbours(lat[rev], np.ones(2), 4)
    assert np.array_equal(vc.to_positions(vc.to_caller(pos, rev), rev), pos)


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
@pytest.mark.parametrize("N,D,k,kernel,fit", vc.VALUE_CASES, ids=lambda v: str(v))
def test_float64_restatement_lies_inside_the_bars_and_is_not_exact(N, D, k, kernel, fit):
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, fit)
    ref = vc.reference(N, D, k, kernel, fit)
    order = ref["order"]
    t80, g80, ok80, _ = vr.terms(c.X[order], c.T[0][order], s, kernel, sigma2, nugget, ref["nbr"], grad=True, fit_nugget=fit, dtype=np.longdouble)
    assert ok80.all()
    et = np.abs(np.asarray(t80 - ref["terms"].astype(np.longdouble), dtype=np.float64))
    g64, gl = ref["grad"].sum(axis=0), np.asarray(g80.sum(axis=0), dtype=np.float64)
    eg = np.abs(g64 - gl)
    print("N %d D %d k %d %s nugget %s: float64 off by at most %.3g (terms) %.3g (gradient), cond at most %.3g"
          % (N, D, k, kernel, "fit" if fit else "fixed", et.max(), eg.max(), ref["cond"].max()))
    # the amplification of every point's own matrix is 1 on these shapes
    assert ref["cond"].max() <= 1e7
    assert et.max() > 0. and vc.excess_rows("logpost", ref["terms"], np.asarray(t80, dtype=np.float64), ref["cond"]) <= 1.
    assert eg.max() > 0. and dc.excess("grad", g64, gl, 1., max(1., float(np.max(np.abs(g64))))) <= 1.


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
class _FakeNative(object):
    calls = 0

    def _no(self, *a, **k):
        _FakeNative.calls += 1
        raise AssertionError("the device must not be reached")

    vecchia_neighbours = vecchia_loglik = predict = _no

    def close(self):
        pass


def test_refusals_come_before_any_device_call(monkeypatch):
    created = []

    def no_device(inputs, residuals, device):
        created.append((inputs.shape, residuals.shape, device))
        return _FakeNative()
    monkeypatch.setattr(VG, "_create_native", no_device)
    rng = np.random.default_rng(0)
    X, t, Q = rng.random((9, 3)), rng.random(9), rng.random((4, 3))
    for b in (np.zeros((9,)), np.zeros((1, 3)), np.zeros((0, 3)), np.zeros((2, 3, 1)), np.zeros((4, 81))):
        with pytest.raises(ValueError, match="inputs must have shape|at most 80 input dimensions"):
            M.VecchiaGP(b, np.zeros(b.shape[0]))
    for bad_t in (np.zeros(8), np.zeros((1, 9)), np.zeros((9, 1))):
        with pytest.raises(ValueError, match="targets must have shape"):
            M.VecchiaGP(X, bad_t)
    for v in (np.nan, np.inf):
        Xb, tb = X.copy(), t.copy()
        Xb[2, 1], tb[3] = v, v
        with pytest.raises(ValueError, match="inputs must be finite"):
            M.VecchiaGP(Xb, t)
        with pytest.raises(ValueError, match="targets must be finite"):
            M.VecchiaGP(X, tb)
    for k in (0, -1, 9, 127, 2.5):
        with pytest.raises(ValueError, match="n_neighbours must be between 1 and"):
            M.VecchiaGP(X, t, n_neighbours=k)
    big = rng.random((200, 3))
    with pytest.raises(ValueError, match=r"n_neighbours must be between 1 and min\(N - 1, 126\) = 126"):
        M.VecchiaGP(big, rng.random(200), n_neighbours=127)
    for order in (np.arange(8), np.zeros(9, dtype=int), np.arange(1, 10), np.arange(9) + 0.5, np.arange(9).reshape(3, 3)):
        with pytest.raises(ValueError, match="order must be a permutation"):
            M.VecchiaGP(X, t, n_neighbours=3, order=order)
    with pytest.raises(ValueError, match="device must be"):
        M.VecchiaGP(X, t, n_neighbours=3, device=-1)
    with pytest.raises(ValueError, match="kernel must be one of"):
        M.VecchiaGP(X, t, n_neighbours=3, kernel="Linear")
    for nug in (-1e-3, np.nan, np.inf, "fixed"):
        with pytest.raises(ValueError, match="nugget must be"):
            M.VecchiaGP(X, t, n_neighbours=3, nugget=nug)
    with pytest.raises(RuntimeError, match="not available with the ProductMat52 kernel"):
        M.VecchiaGP(X, t, n_neighbours=3, kernel="ProductMat52")
    for nug in ("adaptive", "pivot"):
        with pytest.raises(RuntimeError, match='not available with nugget="%s"' % nug):
            M.VecchiaGP(X, t, n_neighbours=3, nugget=nug)
    assert created == []
    order = rng.permutation(9)
    vg = M.VecchiaGP(X, t, kernel="UniformMat52", n_neighbours=3, order=order)
    assert created == [((9, 3), (1, 9), None)] and (vg.n, vg.D, vg.n_neighbours, vg.n_params, vg.kernel) == (9, 3, 3, 3, "UniformMat52")
    assert np.array_equal(vg.order, order)
    fixed = M.VecchiaGP(X, t, n_neighbours=3, nugget=1e-3, rng=1)
    assert fixed.n_params == 4 and np.array_equal(np.sort(fixed.order), np.arange(9))
    assert np.array_equal(fixed.order, M.VecchiaGP(X, t, n_neighbours=3, rng=1).order)
    th = np.zeros(3)
    for bad in (np.zeros(2), np.zeros(4), np.zeros((1, 3))):
        with pytest.raises(ValueError, match="theta must have 3 entries"):
            vg.loglik(bad)
        with pytest.raises(ValueError, match="theta must have 3 entries"):
            vg.set_neighbours(theta=bad)
        with pytest.raises(ValueError, match="theta must have 3 entries"):
            vg.fit(theta0=bad)
    with pytest.raises(ValueError, match="theta must be finite"):
        vg.loglik(np.array([0., np.nan, 0.]))
    with pytest.raises(ValueError, match="does not give positive finite"):
        vg.loglik(np.array([0., 800., 0.]))
    for s in (np.ones(2), np.array([1., 0., 1.]), np.array([1., np.inf, 1.])):
        with pytest.raises(ValueError, match="scales must be 3 positive finite numbers"):
            vg.set_neighbours(scales=s)
    with pytest.raises(ValueError, match="not both"):
        vg.set_neighbours(theta=th, scales=np.ones(3))
    for j in (-1e-300, np.nan, np.inf):
        with pytest.raises(ValueError, match="jitter must be a finite number that is not negative"):
            vg.loglik(th, jitter=j)
    with pytest.raises(ValueError, match="max_points must not be negative"):
        vg.loglik(th, max_points=-1)
    with pytest.raises(RuntimeError, match="set_neighbours has not been called"):
        vg.loglik(th)
    with pytest.raises(RuntimeError, match="set_neighbours has not been called"):
        vg.neighbours
    with pytest.raises(ValueError, match="n_tries must be at least 1"):
        vg.fit(n_tries=0)
    with pytest.raises(ValueError, match="refresh must not be negative"):
        vg.fit(refresh=-1)
    with pytest.raises(RuntimeError, match="fit has not been called"):
        vg.predict(Q)
    with pytest.raises(ValueError, match="n_neighbours must be between 1 and"):
        vg.predict(Q, theta=th, n_neighbours=10)
    with pytest.raises(ValueError, match="testing must have shape"):
        vg.predict(np.zeros((4, 2)), theta=th)
    assert _FakeNative.calls == 0
    vg.close()
    with pytest.raises(RuntimeError, match="has been closed"):
        vg.set_neighbours()
    vg.close()                                    # twice is fine


def test_log_likelihood_bookkeeping():
    ok = np.array([True, False, True])
    ll = M.VecchiaLogLik(-np.inf, None, np.where(ok, 1., np.nan), ok)
    assert ll.n_failed == 1 and ll.grad is None
    best = dict(theta=np.zeros(2), value=1., grad=np.zeros(2), n_evaluations=3, n_refreshes=2, converged=True)
    f = M.VecchiaFit(best, [best])
    assert (f.value, f.n_evaluations, f.n_refreshes, f.converged, len(f.tries)) == (1., 3, 2, True, 1)
