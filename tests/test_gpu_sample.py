"""Joint posterior draws on the MI355X (mogp_emulator_amd.sample_posterior, csrc/kernels_sample.hip) at shapes that sit on the tile
edges: n = 130, D = 3, E = 3 emulators with a different theta each, squared exponential and Matern-5/2, fitted and fixed nugget,
m in {1, 127, 128, 129, 300} query points, S in {1, 3, 65} draws.

Where a bound is not "bit for bit" it is derived, not measured:
  * the identity L L^T = Sigma~ (test 2): the componentwise backward error of a Cholesky factor, (m + 2) 2^-52 sqrt(S_ii S_jj), plus the
    rounding of adding and subtracting mu*, 4 m 2^-52 max|mu*| max sqrt(S_jj);
  * the device against the NumPy restatement (tests 3 and 5): two backward-stable factorisations of one matrix differ to first order by
    4 m 2^-52 cond_2(Sigma~) max sqrt(S_jj), times |z_s|_2 for a draw; cond_2 is computed here by NumPy.
The measured figures are printed next to each bar.
"""
import ctypes
import functools

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import _capi
from mogp_emulator_amd.Priors import GPPriors

import sample_restate as sr

pytestmark = pytest.mark.gpu
EPS = 2. ** -52
N, D, E = 130, 3, 3
MS = (1, 127, 128, 129, 300)
KERNELS = ("SquaredExponential", "Matern52")
NUGGETS = ("fit", 1e-2)
MODELS = [(k, g) for k in KERNELS for g in NUGGETS]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _model_id(mk):
    return "%s-%s" % (mk[0], "fit" if mk[1] == "fit" else "fixed")


def _data():
    rng = np.random.default_rng(77)
    X = rng.random((N, D))
    T = np.array([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 + .1 * rng.standard_normal(N) for k in range(E + 1)])
    return X, T


def _theta(e, fit):
    """correlation lengths of 0.1 - 0.6 times sqrt(D), sigma^2 = e^0.2; a fitted nugget of e^-4 = 0.018 sigma^2 / 1.2"""
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, D) + 0.05 * e
    return np.concatenate([corr, [0.2 + 0.03 * e], [-4. + 0.1 * e] if fit else []])


def _kind(nugget):
    return "fixed" if isinstance(nugget, float) else nugget


@functools.lru_cache(maxsize=None)
def _model(kernel, nugget, n_emulators=E, fit=None, devices=None):
    X, T = _data()
    mo = M.MultiOutputGP_GPU(X, T[:n_emulators], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)),
                             devices=None if devices is None else list(devices))
    for e in (range(n_emulators) if fit is None else fit):
        mo.fit_emulator(e, _theta(e, nugget == "fit"))
    return mo


@functools.lru_cache(maxsize=None)
def _single(kernel, nugget, e):
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[e], kernel=kernel, nugget=nugget, priors=GPPriors(n_corr=D, nugget_type=_kind(nugget)))
    gp.fit(_theta(e, nugget == "fit"))
    return gp


@functools.lru_cache(maxsize=None)
def _points(m):
    return np.random.default_rng(500 + m).random((m, D))


@functools.lru_cache(maxsize=None)
def _reference(kernel, nugget, m):
    """(mu* (E, m), Sigma* (E, m, m), nuggets (E,)) of the model from this build's predict(full_cov=True); computed once, never modified"""
    mo = _model(kernel, nugget)
    p = mo.predict(_points(m), full_cov=True, include_nugget=False, deriv=False)
    for a in (p.mean, p.unc):
        a.setflags(write=False)
    return p.mean, p.unc, np.array(mo._nuggets())


def _tilde(cov, shift):
    return cov + shift * np.eye(cov.shape[0])


def _draw_bar(St, z):
    """per draw: 4 m 2^-52 cond_2(Sigma~) max sqrt(S_jj) |z_s|_2"""
    m = St.shape[0]
    return 4. * m * EPS * np.linalg.cond(St) * np.sqrt(np.max(np.diag(St))) * np.linalg.norm(z, axis=-1)


def _identity_check(samples, mean, St, what):
    """test 2 for one emulator: samples (m, m) of z = I"""
    m = St.shape[0]
    dev = samples - mean[None, :]                    # row k = draw e_k: column k of L
    assert np.all(dev[np.tril_indices(m, -1)] == 0.0), "%s: draw e_k moved a point before k" % what
    Lh = dev.T
    sd = np.sqrt(np.diag(St))
    bound = EPS * ((m + 2) * np.outer(sd, sd) + 4. * m * np.max(np.abs(mean)) * np.max(sd))
    err = np.abs(Lh @ Lh.T - St)
    print("%s: |L L^T - Sigma~| / bound at most %.3g" % (what, np.max(err / bound)))
    assert np.all(err <= bound), (what, float(np.max(err / bound)))


# ---- 1. z = 0 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_zero_normals_return_the_mean_bit_for_bit(mk):
    mo = _model(*mk)
    for m in MS:
        mu, _, _ = _reference(*mk, m)
        for S in (1, 3):
            r = M.sample_posterior(mo, _points(m), z=np.zeros((S, m)))
            assert r.samples.shape == (E, S, m) and r.mean.shape == (E, m) and r.ok.all() and r.seed is None and r.z is None
            assert np.array_equal(r.mean, mu)
            assert np.array_equal(r.samples, np.broadcast_to(mu[:, None, :], (E, S, m))), (mk, m, S)
    one = M.sample_posterior(_single(*mk, 1), _points(129), z=np.zeros((2, 129)))
    assert one.samples.shape == (2, 129) and one.mean.shape == (129,) and one.ok is True
    assert np.array_equal(one.samples[1], _single(*mk, 1).predict(_points(129), full_cov=True, deriv=False).mean)


# ---- 2. z = I ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_identity_normals_return_the_factor(mk, m):
    mo = _model(*mk)
    mu, cov, nug = _reference(*mk, m)
    assert np.all(nug >= 1e-3 * np.exp(0.2))
    r = M.sample_posterior(mo, _points(m), z=np.eye(m), include_nugget=True)
    assert r.ok.all() and np.array_equal(r.jitter_used, np.zeros(E))
    for e in range(E):
        _identity_check(r.samples[e], r.mean[e], _tilde(cov[e], nug[e]), "%s m=%d emulator %d" % (_model_id(mk), m, e))


# ---- 3. against the restatement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("S", (1, 3, 65))
@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_device_matches_the_restatement(mk, S, m):
    """With one point Sigma~ is a scalar and cond_2 = 1: the bar of a draw is 4 * 2^-52 * sqrt(S) * |z_s| (2e-19 - 5e-17 here), below one unit
    in the last place of a sample whose |z_s| is small -- only bit-equal results pass there.  The device meets it because the factor's diagonal
    is finished with the correctly rounded square root (sample_polish_kernel): mu + sqrt(Sigma~) z is then LAPACK's to the bit.  Measured on an
    MI355X: every m = 1 case differs by 0; m >= 127 by at most 2.8e-15, at most 5.6e-4 of the bar."""
    mo = _model(*mk)
    mu, cov, nug = _reference(*mk, m)
    z = np.random.default_rng(31 * m + S).standard_normal((E, S, m))
    r = M.sample_posterior(mo, _points(m), z=z, return_z=True)
    assert r.ok.all() and np.array_equal(r.z, z)
    worst = 0.
    for e in range(E):
        ref, ju, ok, St = sr.sample(mu[e], cov[e], z[e], nugget=nug[e])
        assert ok and ju == 0.
        bar = _draw_bar(St, z[e])
        err = np.max(np.abs(r.samples[e] - ref), axis=-1)
        print("%s m=%d S=%d emulator %d: cond %.3g, device vs restatement at most %.3g, at most %.3g of the bar (smallest bar %.3g)" % (
            _model_id(mk), m, S, e, np.linalg.cond(St), err.max(), np.max(err / bar), bar.min()))
        worst = max(worst, float(np.max(err / bar)))
    # z (S, m) shared by all emulators is the per-emulator form with equal blocks
    shared = M.sample_posterior(mo, _points(m), z=z[0])
    again = M.sample_posterior(mo, _points(m), z=np.broadcast_to(z[0], (E, S, m)))
    assert np.array_equal(shared.samples, again.samples)
    assert worst <= 1., (mk, m, S, worst)


# ---- 4. device normals ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", (1, 127, 128, 129, 300))
def test_device_normals_are_the_restated_generator(m):
    mk, S = MODELS[1], 3
    mo = _model(*mk)
    r = M.sample_posterior(mo, _points(m), n_draws=S, rng=2024, return_z=True)
    assert r.seed == int(np.random.default_rng(2024).integers(0, 2 ** 64, dtype=np.uint64)) and r.z.shape == (E, S, m)
    for e in range(E):
        dis = np.max(np.abs(r.z[e] - sr.normals(r.seed, e, S, m)))
        print("m=%d emulator %d: device normals vs restatement %.3g (bar 1e-13)" % (m, e, dis))
        assert dis <= 1e-13
    for stream in (0, 5):
        one = M.sample_posterior(_single(*mk, 1), _points(m), n_draws=S, rng=2024, stream=stream, return_z=True)
        assert one.seed == r.seed and np.max(np.abs(one.z - sr.normals(r.seed, stream, S, m))) <= 1e-13
    # row e of the model is the single call with stream = e; the model's own stream offset adds to it
    one = M.sample_posterior(_single(*mk, 1), _points(m), n_draws=S, rng=2024, stream=1, return_z=True)
    assert np.array_equal(one.z, r.z[1])
    shifted = M.sample_posterior(mo, _points(m), n_draws=S, rng=2024, stream=4, return_z=True)
    assert np.max(np.abs(shifted.z[1] - sr.normals(r.seed, 5, S, m))) <= 1e-13
    # the normals returned, passed back in, give the same samples bit for bit
    back = M.sample_posterior(mo, _points(m), z=r.z)
    assert np.array_equal(back.samples, r.samples) and np.array_equal(back.mean, r.mean)


# ---- 5. determinism and cutting ------------------------------------------------------------------------------------------------------------

def test_determinism_and_cutting():
    mk, m, S = MODELS[2], 300, 65
    mo = _model(*mk)
    mu, cov, nug = _reference(*mk, m)
    first = M.sample_posterior(mo, _points(m), n_draws=S, rng=9, return_z=True)
    again = M.sample_posterior(mo, _points(m), n_draws=S, rng=9, return_z=True)
    for q in ("samples", "mean", "z", "ok", "jitter_used"):
        assert np.array_equal(getattr(first, q), getattr(again, q)), q
    for max_draws in (1, 7, 0):
        got = M.sample_posterior(mo, _points(m), n_draws=S, rng=9, return_z=True, max_draws=max_draws)
        assert np.array_equal(got.samples, first.samples) and np.array_equal(got.z, first.z), max_draws
    refs = [sr.sample(mu[e], cov[e], first.z[e], nugget=nug[e]) for e in range(E)]
    for max_slots in (1, 3, 0):
        got = M.sample_posterior(mo, _points(m), n_draws=S, rng=9, return_z=True, max_slots=max_slots)
        assert np.array_equal(got.z, first.z) and np.array_equal(got.mean, first.mean) and np.array_equal(got.ok, first.ok)
        print("max_slots=%d: samples bit-equal to the default grouping: %s" % (max_slots, np.array_equal(got.samples, first.samples)))
        for e in range(E):
            err = np.max(np.abs(got.samples[e] - refs[e][0]), axis=-1)
            assert np.all(err <= _draw_bar(refs[e][3], first.z[e])), (max_slots, e)


def test_two_parts_on_one_device_are_the_one_part_model():
    mk, m, S = MODELS[3], 129, 3
    mo, two = _model(*mk), _model(*mk, devices=(0, 0))
    assert len(two.devices) == 2
    mu, cov, nug = _reference(*mk, m)
    a = M.sample_posterior(mo, _points(m), n_draws=S, rng=4, return_z=True)
    b = M.sample_posterior(two, _points(m), n_draws=S, rng=4, return_z=True)
    assert np.array_equal(a.z, b.z) and np.array_equal(a.ok, b.ok)          # the stream offset is the index in the model, not in the part
    print("two parts: samples bit-equal to the one-part model: %s" % np.array_equal(a.samples, b.samples))
    for e in range(E):
        ref, _, _, St = sr.sample(mu[e], cov[e], a.z[e], nugget=nug[e])
        assert np.all(np.max(np.abs(b.samples[e] - ref), axis=-1) <= _draw_bar(St, a.z[e])), e


# ---- 6. the ladder -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mk", MODELS, ids=_model_id)
def test_jitter_ladder_on_a_rank_one_covariance(mk):
    m = 130
    mo = _model(*mk)
    Xs = np.tile(np.array([[0.31, 0.62, 0.47]]), (m, 1))
    p = mo.predict(Xs, full_cov=True, include_nugget=False, deriv=False)
    r = M.sample_posterior(mo, Xs, z=np.eye(m), include_nugget=False, jitter=0.)
    assert r.ok.all() and np.all(np.isfinite(r.samples))
    for e in range(E):
        dbar = np.mean(np.diag(p.unc[e]))
        rungs = [0.] + [sr.ladder_delta(t, dbar) for t in range(sr.LADDER_RUNGS)]
        print("%s emulator %d: mean diagonal %.3g, jitter_used %.3g (rung %s)" % (
            _model_id(mk), e, dbar, r.jitter_used[e], [k - 1 for k, x in enumerate(rungs) if np.isclose(r.jitter_used[e], x, rtol=1e-12, atol=0)]))
        assert r.jitter_used[e] == 0. or any(np.isclose(r.jitter_used[e], x, rtol=1e-12, atol=0) for x in rungs[1:])
        _identity_check(r.samples[e], r.mean[e], _tilde(p.unc[e], r.jitter_used[e]), "%s rank one, emulator %d" % (_model_id(mk), e))
    # with a nugget on the diagonal nothing is added beyond the caller's jitter, exactly
    for jitter in (0., 1e-7):
        q = M.sample_posterior(mo, _points(129), n_draws=2, rng=1, include_nugget=True, jitter=jitter)
        assert q.ok.all() and np.array_equal(q.jitter_used, np.full(E, jitter))


# ---- 7. state and refusals -----------------------------------------------------------------------------------------------------------------

def _counter(name):
    c = ctypes.c_longlong(0)
    assert _capi.load().mogp_profile_counter(name.encode(), ctypes.byref(c)) == 0
    return c.value


def test_engine_state_survives_the_call():
    mk = MODELS[0]
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[0], kernel=mk[0], nugget=mk[1], priors=GPPriors(n_corr=D, nugget_type=_kind(mk[1])))
    gp.fit(_theta(0, True))
    Xs = _points(127)
    th0 = np.concatenate([gp.theta.get_mean(), gp.theta.get_data()])
    lp0, p0 = gp.current_logpost, gp.predict(Xs)
    M.sample_posterior(gp, _points(129), n_draws=3, rng=1)
    live1 = _counter("device_bytes_live")
    M.sample_posterior(gp, _points(129), n_draws=3, rng=1)
    assert _counter("device_bytes_live") == live1                           # the scratch engine and every buffer of the call are gone
    assert np.array_equal(np.concatenate([gp.theta.get_mean(), gp.theta.get_data()]), th0) and gp.current_logpost == lp0
    p1 = gp.predict(Xs)
    assert np.array_equal(p1.mean, p0.mean) and np.array_equal(p1.unc, p0.unc) and np.array_equal(p1.deriv, p0.deriv)


def test_an_emulator_that_is_not_fit():
    mk, m = MODELS[1], 128
    mo = _model(*mk, n_emulators=4, fit=(0, 1, 3))
    full = _model(*mk)
    r = M.sample_posterior(mo, _points(m), n_draws=3, rng=6, return_z=True)
    assert list(r.ok) == [True, True, False, True] and np.isnan(r.jitter_used[2])
    assert np.all(np.isnan(r.samples[2])) and np.all(np.isnan(r.mean[2])) and np.all(np.isfinite(r.samples[[0, 1, 3]]))
    ref = M.sample_posterior(full, _points(m), n_draws=3, rng=6, return_z=True)
    assert np.array_equal(r.z[:2], ref.z[:2]) and np.array_equal(r.mean[:2], ref.mean[:2])          # streams 0 and 1 either way
    assert np.max(np.abs(r.z[3] - sr.normals(r.seed, 3, 3, m))) <= 1e-13                          # the index in the model, not among the fitted
    X, T = _data()
    gp = M.GaussianProcessGPU(X, T[0], kernel=mk[0], nugget=mk[1], priors=GPPriors(n_corr=D, nugget_type="fixed"))
    with pytest.raises(RuntimeError, match="not been fit"):
        M.sample_posterior(gp, _points(m))
    with pytest.raises(RuntimeError, match="not been fit"):
        gp._densegp_gpu.sample_posterior(_points(m))


def test_refusals():
    X, T = _data()
    th = _theta(0, False)
    gp = M.GaussianProcessGPU(X, T[0], nugget="pivot", priors=GPPriors(n_corr=D, nugget_type="pivot"))
    gp.fit(th)
    with pytest.raises(RuntimeError, match="pivot"):
        M.sample_posterior(gp, _points(5))
    with pytest.raises(RuntimeError, match="pivot"):
        gp._densegp_gpu.sample_posterior(_points(5))
    gp = M.GaussianProcessGPU(X, T[0], mean="c+c*x[0]", nugget=1e-4, analytic_mean=True)
    gp.fit(th)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        M.sample_posterior(gp, _points(5))
    with pytest.raises(RuntimeError, match="analytic_mean"):
        gp._densegp_gpu.sample_posterior(_points(5))
    ok = _single(*MODELS[1], 0)
    with pytest.raises(RuntimeError, match="D columns"):
        ok._densegp_gpu.sample_posterior(np.zeros((4, 2)))
    for kw in (dict(n_draws=0), dict(jitter=-1.), dict(max_slots=-1), dict(max_draws=-1), dict(z=np.full((2, 5), np.nan))):
        with pytest.raises((RuntimeError, ValueError)):
            ok._densegp_gpu.sample_posterior(_points(5), **kw)
    bad = _points(5).copy()
    bad[2, 1] = np.inf
    with pytest.raises(RuntimeError, match="finite"):
        ok._densegp_gpu.sample_posterior(bad)
