"""Device memory is owned by the RAII types of csrc/devmem.h, which count the bytes they hold (mogp_profile_counter
"device_bytes_live").  Every handle gives back what it took, on the normal path and on an error path, through one part or several.

Only differences of the counter are compared, never its value: other tests of the same process may hold models alive.

fit_GP_MAP keeps one replica engine per device for the next fit of the same shape, and an engine allocates some buffers at their first
use (L^-1, the pivot buffers, the packs of the one-launch Cholesky).  So a round is repeated with a fixed optimiser seed: after a
warm-up round, every further round ends with exactly the bytes the warm-up round ended with.

The fused implausibility serves zero / fixed mean functions only; on the analytic-mean model the call is made all the same and must
raise, which is one more error path that has to give everything back."""
import ctypes
import gc

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, _capi

pytestmark = pytest.mark.gpu

N, D, NE = 130, 3, 3          # n = 130: two 128-row tiles (NP = 256)
NP = 256
M_FULL, N_SOBOL = 40, 64


def live():
    c = ctypes.c_longlong(-1)
    assert _capi.load().mogp_profile_counter(b"device_bytes_live", ctypes.byref(c)) == 0
    return c.value


def _data():
    rng = np.random.default_rng(5)
    X = rng.uniform(0., 1., (N, D))
    T = np.stack([np.sin(2.5 * X @ rng.normal(size=D)) + 0.3 * k + 0.01 * rng.normal(size=N) for k in range(NE)])
    Xs = rng.uniform(0., 1., (M_FULL, D))
    A, B = rng.uniform(0., 1., (N_SOBOL, D)), rng.uniform(0., 1., (N_SOBOL, D))
    return X, T, Xs, A, B


X, T, XS, SA, SB = _data()
OBS, OBS_VAR, DISC = np.array([0.1, 0.4, 0.7]), np.full(NE, 0.01), np.full(NE, 0.02)

MODELS = {
    "plain": dict(),
    "analytic_mean": dict(mean="c", analytic_mean=True),
    "two_parts": dict(devices=[0, 0]),
}


def _thetas(gp):
    nm = gp._mogp_gpu.emulator(0).get_theta().get_n_mean()
    return np.array([np.concatenate([0.1 * np.ones(nm), [-1.2 + 0.1 * k, -0.8, -0.5 + 0.05 * k], [0.2 - 0.03 * k]]) for k in range(NE)])


def _matrices(native):
    n = native.n()
    for fill in (native.get_K, native.get_invQ, native.get_cholesky_lower):
        out = np.zeros((n, n))
        fill(out)
        assert np.isfinite(out).all()
    assert np.isfinite(native.loo_variance()).all()


def exercise_multi(kind):
    gp = M.MultiOutputGP_GPU(X, T, **MODELS[kind])
    assert gp._mogp_gpu.n_parts() == (2 if kind == "two_parts" else 1)
    th = _thetas(gp)
    f, g, ok = gp._mogp_gpu.eval(th, grad=True)
    assert ok.all() and np.isfinite(f).all() and np.isfinite(g).all()
    gp.fit(th)
    # one emulator left unfitted: the fitted rows are computed on compact scratch and scattered
    gp._mogp_gpu.emulator(2).reset_theta_fit_status()
    assert gp.get_indices_not_fit() == [2]
    r = gp.predict(XS, unc=True, deriv=True, allow_not_fit=True)
    assert np.isfinite(r.mean[:2]).all() and np.isfinite(r.unc[:2]).all() and np.isfinite(r.deriv[:2]).all()
    r = gp.predict(XS, unc=True, deriv=False, allow_not_fit=True, full_cov=True)
    assert r.unc.shape == (NE, M_FULL, M_FULL) and np.isfinite(r.unc[:2]).all()
    S, ST, mu, var, ev = gp._mogp_gpu.sobol(SA, SB, unc=True)
    assert np.isfinite(S[:2]).all() and np.isfinite(ev[:2]).all() and np.isnan(S[2]).all() and np.isnan(ev[2])
    gp.fit_emulator(2, th[2])
    assert gp.get_indices_not_fit() == []
    if kind == "analytic_mean":
        with pytest.raises(RuntimeError, match="zero / fixed mean functions only"):
            gp._mogp_gpu.implausibility(XS, OBS, OBS_VAR, DISC, rank=1)
    else:
        assert np.isfinite(gp._mogp_gpu.implausibility(XS, OBS, OBS_VAR, DISC, rank=1)).all()
    _matrices(gp._mogp_gpu.emulator(0))
    gp = M.fit_GP_MAP(gp, n_tries=2)
    assert gp.get_indices_not_fit() == []


def exercise_pivot():
    Xr = X.copy()
    Xr[N - 1] = Xr[0]                      # one repeated input: the pivoted factorisation stops below n
    gp = M.GaussianProcessGPU(Xr, np.sin(2.5 * Xr[:, 0]) + Xr[:, 1], nugget="pivot")
    th = np.array([-1.2, -0.8, -0.5, 0.2])
    assert np.isfinite(gp.logpost_deriv(th)).all()      # fit + gradient: the rows of L^-1 of the skipped pivots are held apart
    assert gp.pivot_rank < N
    r = gp.predict(XS, unc=True, deriv=True)
    assert np.isfinite(r.mean).all() and np.isfinite(r.unc).all() and np.isfinite(r.deriv).all()
    r = gp.predict(XS, unc=True, deriv=False, full_cov=True)
    assert r.unc.shape == (M_FULL, M_FULL)
    native = gp._densegp_gpu
    assert np.isfinite(native.implausibility(XS, 0.3, 0.01, 0.02)).all()      # a single output: rank 0 is the only one there is
    S, ST, mu, var, ev = native.sobol(SA, SB, unc=True)
    assert np.isfinite(S).all() and np.isfinite(ev)
    _matrices(native)
    gp = M.fit_GP_MAP(gp, n_tries=2)
    assert gp.theta.data_has_been_set()


def one_round():
    LibGPGPU.set_fit_options(seed=7)       # every round draws the same starts: the same buffers come into use
    for kind in MODELS:
        exercise_multi(kind)
    exercise_pivot()
    gc.collect()
    return live()


def test_every_handle_gives_back_what_it_took():
    try:
        warm = one_round()
        for _ in range(2):
            assert one_round() == warm
    finally:
        LibGPGPU.set_fit_options(seed=0)


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_error_after_the_scratch_is_allocated_gives_it_back(devices):
    gp = M.MultiOutputGP_GPU(X, T, devices=devices)
    gp.fit(_thetas(gp))
    good = gp._mogp_gpu.implausibility(XS, OBS, OBS_VAR, DISC, rank=1)      # (the prediction scratch of the engines is in place)
    before = live()
    with pytest.raises(RuntimeError, match="discrepancy variance cannot be negative"):
        gp._mogp_gpu.implausibility(XS, OBS, OBS_VAR, np.array([0.02, -0.02, 0.02]), rank=1)
    assert live() == before
    again = gp._mogp_gpu.implausibility(XS, OBS, OBS_VAR, DISC, rank=1)
    assert live() == before
    np.testing.assert_array_equal(again, good)


def test_the_counter_follows_a_model():
    gp = M.MultiOutputGP_GPU(X, T)
    gp.fit(_thetas(gp))
    held = live()
    del gp
    gc.collect()
    assert held - live() >= 8 * NE * NP * NP
