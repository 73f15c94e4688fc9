"""gKDR on the MI355X: the reference's tests/test_DimensionReduction.py ported, the golden cases under the R and B bounds (units of
cond_2(A) eps, eps = 2^-52), grid against one-at-a-time construction, bitwise reproducibility over pass sizes and runs, the tuning
search, and matrices that are not positive definite."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import DimensionReduction as DR
from mogp_emulator_amd import fitting
from mogp_emulator_amd.DimensionReduction import gKDR, gram_matrix, gram_matrix_sqexp, median_dist

from gkdr_restate import R_exact, check_B, cond2, eig_sorted, lstsq_model, scales2

pytestmark = pytest.mark.gpu
EPS64 = 2.0 ** -52


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


# ---- the reference's tests/test_DimensionReduction.py ------------------------------------------------------------------------
def fn(x):
    return 10 * (x[0] + x[1]) + (x[1] - x[0])


def fn3(x):
    return x[0]


def test_DimensionReduction_basic():
    Y = np.array([[1], [2.1], [3.2]])
    X = np.array([[1, 2, 3], [4, 5.1, 6], [7.1, 8, 9.1]])
    dr = gKDR(X, Y, K=2, SGX=2, SGY=2, EPS=1E-5)
    assert dr.K == 2


def test_DimensionReduction_tune_parameters():
    np.random.seed(100)
    X = np.random.random((20, 20))
    Y = np.apply_along_axis(fn3, 1, X)
    dr, loss = gKDR.tune_parameters(X, Y, fitting.fit_GP_MAP, cXs=[5.0], cYs=[5.0], maxK=3)
    assert dr.K <= 2
    assert 0.0 < loss < 0.2


def test_DimensionReduction_GP():
    X = np.mgrid[0:10, 0:10].T.reshape(-1, 2) / 10.0
    Y = np.apply_along_axis(fn, 1, X)
    dr = gKDR(X, Y, 1)
    np.random.seed(10)
    gp = fitting.fit_GP_MAP(X, Y)
    gp_red = fitting.fit_GP_MAP(dr(X), Y)
    Xnew = (np.mgrid[0:9, 0:9].T.reshape(-1, 2) + 0.5) / 10.0
    Yexpect = np.apply_along_axis(fn, 1, Xnew)
    assert np.max(np.abs(gp.predict(Xnew)[0] - Yexpect)) <= 0.02
    assert np.max(np.abs(gp_red.predict(dr(Xnew))[0] - Yexpect)) <= 0.02


def test_DimensionReduction_B():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    Y = np.array([0.1, 1.0, 3.0, 3.6])
    dr = gKDR(X, Y, 2, SGX=1.0, SGY=2.0)
    B_expected = np.array([[-0.2653073259794961, -0.9641638982982144],
                           [-0.9641638982982144, 0.2653073259794961]])
    for i in range(B_expected.shape[1]):
        r = dr.B[:, i] / B_expected[:, i]
        assert np.allclose(r, 1.0) or np.allclose(r, -1.0)


def test_DimensionReduction_median_dist():
    assert np.allclose(median_dist(np.array([[0.0], [1.0], [2.0]])), 1)
    assert np.allclose(median_dist(np.array([[0.0], [1.0], [2.0], [3.0]])), 1.5)


def test_DimensionReduction_gram_matrix():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])

    def k_sqexp(x0, x1):
        d = x0 - x1
        return np.exp(-0.5 * np.dot(d, d))
    G_dot = gram_matrix(X, lambda a, b: np.dot(a, b))
    assert np.allclose(G_dot, np.array([[0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 2.0]]))
    expected = np.exp(np.array([[0.0, -0.5, -0.5, -1.0], [-0.5, 0.0, -1.0, -0.5], [-0.5, -1.0, 0.0, -0.5], [-1.0, -0.5, -0.5, 0.0]]))
    assert np.allclose(gram_matrix_sqexp(X, 1.0), expected)
    assert np.allclose(gram_matrix(X, k_sqexp), expected)


def test_DimensionReduction_large():
    X = np.eye(200, 3200)
    Y = np.arange(200)
    dr = gKDR(X, Y, 2)
    assert dr.B.shape == (3200, 3200) and np.all(np.isfinite(dr.R))


# ---- golden cases --------------------------------------------------------------------------------------------------------------
def _case(g, name):
    kw = {}
    for k in ["X_scale", "Y_scale", "EPS", "SGX", "SGY"]:
        v = float(g[name + "_" + k])
        if not np.isnan(v):
            kw[k] = v
    return g[name + "_X"], g[name + "_Y"], kw


@pytest.mark.parametrize("name", ["n200", "n300_off", "sg", "eps0", "n1000", "n2000"])
def test_golden_R_and_B(golden, name):
    g = golden("gkdr.npz")
    X, Y, kw = _case(g, name)
    dr = gKDR(X, Y, **kw)
    sx, sy = scales2(X, Y, kw.get("X_scale", 1.0), kw.get("Y_scale", 1.0), kw.get("SGX"), kw.get("SGY"))
    eps = kw.get("EPS", 1e-8)
    ce = cond2(X, sx, eps) * EPS64
    R_ref = g[name + "_R"]
    if X.shape[0] <= 300:
        R_ex = R_exact(X, Y, sx, sy, eps).astype(np.float64)
        err = np.linalg.norm(dr.R - R_ex) / np.linalg.norm(R_ex)
        assert err <= 20 * ce, (err, ce)
    else:
        err = np.linalg.norm(dr.R - R_ref) / np.linalg.norm(R_ref)
        assert err <= 40 * ce, (err, ce)
    eig_ref, B_ref = eig_sorted(R_ref)
    assert np.array_equal(dr.B, eig_sorted(dr.R)[1])
    assert check_B(dr.B, g[name + "_B"], dr.R, R_ref, eig_ref) >= 1


def test_grid_agrees_with_one_at_a_time(golden):
    g = golden("gkdr.npz")
    X, Y = g["n200_X"], g["n200_Y"]
    cXs, cYs = [0.5, 1.0, 5.0], [0.5, 2.0]
    n0 = gKDR.device_calls
    drs = gKDR.grid(X, Y, cXs, cYs, K=2)
    assert gKDR.device_calls - n0 == 1
    assert len(drs) == 6
    for i, cX in enumerate(cXs):
        for j, cY in enumerate(cYs):
            dr, one = drs[i * len(cYs) + j], gKDR(X, Y, 2, cX, cY)
            assert (dr.K, dr.X_scale, dr.Y_scale) == (2, cX, cY)
            # the same scales reach the device, and a pair's R does not depend on the other pairs of the call
            assert np.array_equal(dr.R.view(np.uint64), one.R.view(np.uint64))
            assert np.array_equal(dr.B, one.B)
            np.testing.assert_allclose(dr(X), dr.__call__(X))


def test_R_is_bitwise_independent_of_the_pass_size_and_the_run(golden):
    g = golden("gkdr.npz")
    X, Y = g["n300_off_X"], g["n300_off_Y"]
    sx = [scales2(X, Y, c)[0] for c in (0.5, 1.0, 5.0)]
    sy = [scales2(X, Y, 1.0, c)[1] for c in (0.5, 1.0, 5.0)]
    R_auto, info = DR.device_R(X, Y, sx, sy, 1e-8, 0)
    R_one, info1 = DR.device_R(X, Y, sx, sy, 1e-8, 1)
    R_two, _ = DR.device_R(X, Y, sx, sy, 1e-8, 2)
    R_again, _ = DR.device_R(X, Y, sx, sy, 1e-8, 0)
    assert not info.any() and not info1.any()
    assert np.all(np.isfinite(R_auto))
    for other in (R_one, R_two, R_again):
        assert np.array_equal(R_auto.view(np.uint64), other.view(np.uint64))
    # a pair's R does not depend on the other pairs of the call
    R_single, _ = DR.device_R(X, Y, sx[1:2], sy[2:3], 1e-8, 0)
    assert np.array_equal(R_single[0, 0].view(np.uint64), R_auto[1, 2].view(np.uint64))


def test_tune_parameters_matches_the_reference_search(golden):
    g = golden("gkdr.npz")
    n0 = gKDR.device_calls
    seq = []
    orig = gKDR.tune_parameters
    dr, loss = orig(g["tune_X"], g["tune_Y"], lambda X, Y: (seq.append(X.shape), lstsq_model(X, Y))[1], maxK=4)
    # one device call per fold, one for the final object
    assert gKDR.device_calls - n0 == 5 + 1
    ref = g["tune_seq"]
    assert len(seq) == 5 * len(ref)
    assert [s[1] for s in seq] == [int(k) for k in ref[:, 0] for _ in range(5)]
    assert (dr.K, dr.X_scale, dr.Y_scale) == tuple(g["tune_argmin"])
    assert loss == pytest.approx(float(g["tune_loss"]), rel=1e-7)


def test_tune_parameters_losses_match_the_reference(golden, capsys):
    g = golden("gkdr.npz")
    gKDR.tune_parameters(g["tune_X"], g["tune_Y"], lstsq_model, maxK=4, verbose=True)
    lines = capsys.readouterr().out.strip().splitlines()
    ref = g["tune_seq"]
    assert len(lines) == len(ref)
    for line, (k, cX, cY, loss) in zip(lines, ref):
        head, val = line.split(" = ")
        assert head == "loss(K={}, X_scale={}, Y_scale={})".format(int(k), cX, cY)
        assert float(val) == pytest.approx(loss, rel=1e-7)


def test_not_positive_definite(golden):
    g = golden("gkdr.npz")
    # rows 0 and 1 equal, EPS = 0: the second pivot is exactly 0 (the reference's cho_factor raises on this input)
    with pytest.raises(np.linalg.LinAlgError):
        gKDR(g["dup_X"], g["dup_Y"], EPS=0.0)
    # one call with scales so large that Kx is the all-ones matrix (not positive definite at EPS = 0) around well-posed ones: the
    # failing scales come first, so that a factored scale's place among the factored ones differs from its place in the call
    X, Y, kw = _case(g, "eps0")
    sx, sy = scales2(X, Y, 0.2)
    sx2 = scales2(X, Y, 0.3)[0]
    R, info = DR.device_R(X, Y, [1e40 * sx, sx, 1e40 * sx, sx2], [sy, 4 * sy], 0.0)
    assert list(info) == [1, 0, 1, 0]
    assert np.all(np.isnan(R[0])) and np.all(np.isnan(R[2]))
    for i, s2 in [(1, sx), (3, sx2)]:
        for j, t2 in enumerate([sy, 4 * sy]):
            alone, info1 = DR.device_R(X, Y, [s2], [t2], 0.0)
            assert list(info1) == [0]
            assert np.array_equal(alone[0, 0].view(np.uint64), R[i, j].view(np.uint64))
    ce = cond2(X, sx, 0.0) * EPS64
    R_ex = R_exact(X, Y, sx, sy, 0.0).astype(np.float64)
    assert np.linalg.norm(R[1, 0] - R_ex) <= 20 * ce * np.linalg.norm(R_ex)
    with pytest.raises(np.linalg.LinAlgError):
        gKDR.grid(X, Y, [0.2, 1e20], [1.0], EPS=0.0)
