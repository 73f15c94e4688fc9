"""The identity padding below the last real row (rows >= n + R of an emulator's NP x NP matrix, NP = roundup(n + R, 128)) is skipped by the
one-launch Cholesky's row tiles and by the triangular inverse (csrc/chol_schedule.h real_rows; kernels_mchol.hip, trsm_dev.h, kernels_gemm.hip,
kernels_chol.hip).  Small designs whose real rows end 0, 1, 15, 16, 32, 48, 64, 65, 128, 129 and 145 rows into the last 128-row block: every
count of real 16-row sub-tiles of a 64-row tile, tiles with no real row, and a last block column that is all padding but one row -- at
NP = 384 and 512, so that there are panel tasks below the diagonal block (two block columns and more) and diagonal-tile GEMM tasks (three
and more).

Bars: those DESIGN section 4 states -- log-posterior rtol 1e-10, gradient rtol 1e-7 (atol 1e-7 of its largest entry), mean rtol 1e-7 (atol 1e-8
as test_gpu_parity), variance atol 1e-7 sigma^2; K^-1 t rtol 1e-6 / atol 1e-6 of its largest entry and K^-1 K = I to 1e-8 as test_gpu_parity
holds them.  The analytic-mean case takes the bars of test_gpu_parity.test_analytic_mean_multioutput_tile_boundaries.

No getter of the C ABI reaches rows >= n of the factor or of L^-1, so the sentinel test holds what the getters do reach: a stale or
damaged padding row would enter the next evaluation's products (the buffers are reused), and the second and third evaluation are held to
the oracle and to the first."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

ETA = 1e-4
D = 2
M_PRED = 64
B_MAX = 16
SIZES = [255, 256, 270, 271, 287, 303, 319, 320, 383, 384, 400]
BATCHES = [1, 3, 16]
THETA_A = np.array([4.0, 3.5, 0.0])
THETA_B = np.array([3.0, 4.5, 0.3])


def _weak():
    return GPPriors(n_corr=D, nugget_type="fixed")


@functools.lru_cache(maxsize=None)
def _data(n):
    rng = np.random.default_rng(9000 + n)
    X = rng.uniform(0., 1., (n, D))
    X.setflags(write=False)
    w = rng.normal(size=(B_MAX, D))
    T = np.stack([np.sin(3. * X @ w[k]) + 0.3 * k * X[:, 0] + 0.01 * rng.normal(size=n) for k in range(B_MAX)])
    T.setflags(write=False)
    Xs = rng.uniform(0., 1., (M_PRED, D))
    Xs.setflags(write=False)
    return X, T, Xs


@functools.lru_cache(maxsize=None)
def _oracle(n, k, which):
    """(logpost, gradient, K^-1 t, K + eta I, mean, variance) of emulator k at theta A or B; computed once, read-only"""
    X, T, Xs = _data(n)
    theta = THETA_A if which == "A" else THETA_B
    ref = R.GPRef(X, T[k], nugget=ETA)
    f = float(ref.fit(theta))
    g = np.array(ref.logpost_deriv(theta))
    mu, var, _ = ref.predict(Xs)
    out = (f, g, np.array(ref.Kinv_t), ref.get_K_matrix() + ETA * np.eye(n), np.array(mu), np.array(var))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _device(n, B):
    """one model of the first B outputs: eval with the gradient at theta A, fit, predict, the getters of its first and last emulator"""
    X, T, Xs = _data(n)
    mo = M.MultiOutputGP_GPU(X, T[:B], nugget=ETA, priors=_weak())
    thetas = np.tile(THETA_A, (B, 1))
    f, g, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    Q = {}
    for k in sorted({0, B - 1}):
        Q[k] = np.zeros((n, n))
        mo._mogp_gpu.emulator(k).get_invQ(Q[k])
    mo.fit(thetas)
    alpha = {k: np.array(mo.emulators[k].Kinv_t) for k in sorted({0, B - 1})}
    mean, unc, _ = mo.predict(Xs, deriv=False)
    return dict(f=np.array(f), g=np.array(g), Q=Q, alpha=alpha, mean=np.array(mean), unc=np.array(unc))


def _hold_to_oracle(n, k, f, g, alpha, Q, mean, unc, which="A"):
    rf, rg, ra, Kn, rmu, rvar = _oracle(n, k, which)
    sigma2 = np.exp((THETA_A if which == "A" else THETA_B)[D])
    print("n=%d k=%d %s: logpost %.2e  grad %.2e of max  alpha %.2e of max  mean %.2e  var %.2e sigma^2" % (
        n, k, which, abs(f - rf) / abs(rf), np.abs(g - rg).max() / np.abs(rg).max(),
        np.abs(alpha - ra).max() / np.abs(ra).max() if alpha is not None else -1.,
        np.abs(mean - rmu).max() if mean is not None else -1., np.abs(unc - rvar).max() / sigma2 if unc is not None else -1.))
    assert_allclose(f, rf, rtol=1e-10)
    assert_allclose(g, rg, rtol=1e-7, atol=1e-7 * np.abs(rg).max())
    if alpha is not None:
        assert_allclose(alpha, ra, rtol=1e-6, atol=1e-6 * np.abs(ra).max())
    if Q is not None:
        assert_allclose(Q @ Kn, np.eye(n), atol=1e-8)
        assert_allclose(Q, Q.T, atol=0)
    if mean is not None:
        assert_allclose(mean, rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(unc, rvar, atol=1e-7 * sigma2)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", SIZES)
def test_padding_edges_against_the_oracle(n, B):
    """log-posterior, gradient, K^-1 t, K^-1 and the prediction at 64 points of the first and the last emulator of the batch"""
    dev = _device(n, B)
    for k in sorted({0, B - 1}):
        _hold_to_oracle(n, k, dev["f"][k], dev["g"][k], dev["alpha"][k], dev["Q"][k], dev["mean"][k], dev["unc"][k])


@pytest.mark.parametrize("n", SIZES)
def test_batch_of_one_equals_its_row_of_sixteen(n):
    """the same emulator alone and as row 0 of sixteen (one queue against eight): the same bits"""
    one, many = _device(n, 1), _device(n, 16)
    assert np.array_equal(one["f"][0], many["f"][0])
    assert np.array_equal(one["g"][0], many["g"][0])
    assert np.array_equal(one["alpha"][0], many["alpha"][0])
    assert np.array_equal(one["Q"][0], many["Q"][0])
    assert np.array_equal(one["mean"][0], many["mean"][0])
    assert np.array_equal(one["unc"][0], many["unc"][0])


@pytest.mark.parametrize("n", [270, 319])
def test_two_workgroups_per_cu_build(n):
    """512 emulators of NP = 384 are past the launcher's threshold for two workgroups per CU (rho >= 1.2: kernels_mchol.hip launch_mchol), the
    other build of the kernel: 15 real rows in the last row tile (n = 270: the half-height GEMM) and a last row tile without a real row
    (n = 319).  Sixteen different targets thirty-two times over; the first and the last emulator against the oracle."""
    X, T, Xs = _data(n)
    B = 512
    mo = M.MultiOutputGP_GPU(X, np.tile(T, (B // B_MAX, 1)), nugget=ETA, priors=_weak())
    f, g, ok = mo._mogp_gpu.eval(np.tile(THETA_A, (B, 1)), grad=True)
    assert ok.all()
    Q = np.zeros((n, n))
    mo._mogp_gpu.emulator(B - 1).get_invQ(Q)
    _hold_to_oracle(n, 0, f[0], g[0], None, None, None, None)
    _hold_to_oracle(n, B_MAX - 1, f[B - 1], g[B - 1], None, Q, None, None)
    # copies of one emulator in different queues and ticket groups: the same bits
    assert np.array_equal(f[:B_MAX], f[B - B_MAX:]) and np.array_equal(g[:B_MAX], g[B - B_MAX:])


def test_analytic_mean_rows_end_in_a_sub_tile_of_right_hand_sides():
    """n = 270 with an intercept and one linear term: R = 3, n + R = 273 -- the second 16-row sub-tile of the last real row tile holds
    the last right-hand-side row and nothing else"""
    n, B = 270, 3
    X, T, Xs = _data(n)
    terms = [(0, 1)]
    mo = M.MultiOutputGP_GPU(X, T[:B], mean=LibGPGPU.PolyMeanFunc(terms), nugget=ETA, priors=_weak(), analytic_mean=True)
    thetas = np.tile(THETA_A, (B, 1))
    f, g, ok = mo._mogp_gpu.eval(thetas, grad=True)
    assert ok.all()
    mo.fit(thetas)
    mean, unc, _ = mo.predict(Xs, deriv=False)
    for k in range(B):
        ref = R.GPRefMean(X, T[k], terms, True, nugget=ETA)
        assert_allclose(f[k], ref.fit(THETA_A), rtol=1e-9)
        assert_allclose(g[k], ref.logpost_deriv(THETA_A), rtol=1e-6, atol=1e-6)
        rmu, rvar, _ = ref.predict(Xs)
        assert_allclose(mean[k], rmu, rtol=1e-7, atol=1e-8)
        assert_allclose(unc[k], rvar, rtol=1e-6, atol=1e-9)
        assert_allclose(mo._mogp_gpu.emulator(k).get_beta(), ref.beta, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("n", [270, 319, 384])
def test_padding_survives_repeated_evaluations(n):
    """theta A, theta B, theta A again on one engine (the factor, L^-1 and K^-1 buffers are reused and the skipped sub-tiles are written
    with their zeros every time): B against the oracle, the third evaluation the first one's bits; then the factor through its getter:
    an exactly zero upper triangle and L L^T = K + eta I to 1e-12 (test_gpu_parity's bar)"""
    X, T, Xs = _data(n)
    B = 3
    mo = M.MultiOutputGP_GPU(X, T[:B], nugget=ETA, priors=_weak())
    fa, ga, ok = mo._mogp_gpu.eval(np.tile(THETA_A, (B, 1)), grad=True)
    assert ok.all()
    fa, ga = np.array(fa), np.array(ga)
    fb, gb, ok = mo._mogp_gpu.eval(np.tile(THETA_B, (B, 1)), grad=True)
    assert ok.all()
    Q = np.zeros((n, n))
    mo._mogp_gpu.emulator(B - 1).get_invQ(Q)
    _hold_to_oracle(n, B - 1, fb[B - 1], gb[B - 1], None, Q, None, None, which="B")
    fc, gc, ok = mo._mogp_gpu.eval(np.tile(THETA_A, (B, 1)), grad=True)
    assert ok.all()
    assert np.array_equal(fa, fc) and np.array_equal(ga, gc)
    mo.fit(np.tile(THETA_A, (B, 1)))
    L = mo.emulators[0].L
    assert np.all(np.triu(L, 1) == 0.)
    assert np.abs(L @ L.T - _oracle(n, 0, "A")[3]).max() < 1e-12
