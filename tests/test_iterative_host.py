"""Host-side checks of the iterative exact prediction (mogp_emulator_amd.IterativeGP): the plan, the memory refusal and every refusal text of
csrc/predict_plan.h through a sanitised stand-alone program (tests/c/iter_plan_check.cpp), the argument refusals that need no device, and
the NumPy restatement (iterative_restate.py) against itself:

* its solve agrees with np.linalg.solve to its own reported residual, and freezes every column on its own;
* at rtol = 1e-10 it converges, on every shape the GPU tests solve on, within 600 iterations -- the GPU tests allow 1000, so the cap never
  hides a device failure;
* its float64 product lies inside the bar the device's product is held to (test_gpu_iterative.py) and is not exact: the bar is not vacuous.

SOLVE_SHAPES, MATVEC_SHAPES, the right-hand sides and the bar are defined here and imported by test_gpu_iterative.py."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")    # the module: the package exports the class under the same name

import dimension_cases as dc
import iterative_restate as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA2 = float(np.exp(dc.LOG_COV))
RTOL, MAX_ITER, ITER_CAP = 1e-10, 1000, 600
FOUR = ["SquaredExponential", "Matern52", "UniformSqExp", "UniformMat52"]

# (n, D, kernel, precond_rank): the shapes the solver is run on, with the iteration counts of this restatement's algorithm in the issue's table
SOLVE_SHAPES = [(300, 3, "SquaredExponential", 64), (300, 3, "SquaredExponential", 0), (300, 3, "Matern52", 64),
                (1000, 5, "SquaredExponential", 256), (1000, 5, "UniformSqExp", 128), (130, 17, "SquaredExponential", 32),
                (130, 80, "Matern52", 32), (130, 1, "SquaredExponential", 32)]
# (n, D, kernel, precond_rank) of the GPU tests that predict: the target row and all 37 cross columns go through the solver
PREDICT_SHAPES = [(n, D, k, p) for n, D, p in ((300, 3, 64), (1000, 5, 256)) for k in ("SquaredExponential", "Matern52")]
LINEAR_MEAN = (300, 3, "Matern52", 64, np.array([0.7, -1.3]))      # the shape and the fixed coefficients c + c x[0] of the mean-function test
MULTI = (300, 3, "SquaredExponential", 64, 3, 9)                    # n, D, kernel, p, emulators, queries of the multi-output test
# (N, D, r, kernels) of the square product
MATVEC_SHAPES = ([(130, 3, r, FOUR) for r in (1, 7, 16, 17, 33)] + [(126, 2, 16, FOUR), (300, 3, 16, FOUR), (1000, 5, 32, FOUR)]
                 + [(130, D, 16, FOUR) for D in (1, 16, 17, 32, 33, 79, 80)])
MATVEC_CASES = [(N, D, r, k) for N, D, r, ks in MATVEC_SHAPES for k in ks]


def setup(n, D, kernel, m=dc.M_TEST[0], E=1):
    """(case, scales per emulator) at the hyperparameters of dimension_cases: fixed nugget 1e-4, sigma^2 = e^0.1"""
    c = dc.case(n, D, kernel, m=m, E=E)
    return c, [ir.scales(c.thetas[e][:c.nc], D, kernel) for e in range(E)]


def right_hand_sides(c, s, kernel):
    """the target row and seven cross columns, (n, 8)"""
    return np.ascontiguousarray(np.column_stack([c.T[0], ir.covariance(c.X, c.Xs[:7], s, kernel, SIGMA2)]))


def matvec_input(N, r, seed=0):
    return np.random.default_rng([seed, N, r]).standard_normal((N, r))


def matvec_bar(Aabs, V, D):
    """per entry (i, c): 2^-52 [(N + 4) sum_j |A_ij| |V_jc| + (4 D + 32) sigma^2 sum_j |V_jc|] -- a fixed-order sum of N products, and the
    absolute error of one generated entry ((D + 2) roundings of the difference-form r2 reach k through k r2 / 2 <= 1 / e; the rest is the
    table exponential's)"""
    N = V.shape[0]
    return 2. ** -52 * ((N + 4) * (Aabs @ np.abs(V)) + (4 * D + 32) * SIGMA2 * np.abs(V).sum(axis=0)[None, :])


def _build_and_run(tmp_path, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_plan_memory_refusal_and_refusal_texts(tmp_path):
    out = _build_and_run(tmp_path, "iter_plan_check")
    assert out.strip() == "ok 53 checks"


def test_panel_transposes_follow_the_index_formula_and_stay_inside_their_window(tmp_path):
    """tests/c/iter_panel_check.cpp: csrc/iter_panel.h both ways at (N, r) = (1, 1), (5, 33), (130, 7), the windows of the passes of 32 and of
    the probe columns, leading dimensions beyond the counts, canaries around the destination"""
    out = _build_and_run(tmp_path, "iter_panel_check")
    assert out.strip() == "ok 48 checks"


def test_exports():
    assert M.IterativeGP is IG.IterativeGP and M.IterativeSolve is IG.IterativeSolve and M.IterativePrediction is IG.IterativePrediction
    assert hasattr(M.VecchiaGP, "predict_exact")
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        names = ("mogp_local_kmatvec", "mogp_local_precondition", "mogp_local_solve", "mogp_local_predict_exact")
        header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
        for name in names:
            assert name in _capi.SIGNATURES and name + "(" in header
        for method in ("kmatvec", "precondition", "solve", "predict_exact"):
            assert hasattr(LibGPGPU.LocalGP_GPU, method)


def test_not_a_gpu_emulator_is_refused():
    for bad in (None, object(), np.zeros(3), "gp"):
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.IterativeGP(bad, np.zeros((4, 2)), np.zeros(4))


class _NoDevice(object):
    """stands for the native handle; anything that would go to the device is an error"""
    calls = 0

    def _touch(self, *a, **k):
        _NoDevice.calls += 1
        raise AssertionError("the device must not be reached")

    kmatvec = precondition = solve = predict_exact = _touch

    def close(self):
        pass


def test_refusals_of_a_view_come_before_any_device_call():
    good = [(0, np.ones(3), 1.1, 1e-4, None, np.zeros(0))]
    for p in (-1, 10, 2.5):
        with pytest.raises(ValueError, match=r"precond_rank must be between 0 and min\(N, 1024\) = 9"):
            M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=p)
    with pytest.raises(ValueError, match=r"precond_rank must be between 0 and min\(N, 1024\) = 1024"):
        M.IterativeGP._on_handle(_NoDevice(), good, 3, 5000, precond_rank=1025)
    for r in (0., 1., -1e-3, 2., np.nan, np.inf):
        with pytest.raises(ValueError, match="rtol must lie between 0 and 1"):
            M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=4, rtol=r)
    for it in (0, -1, 2.5):
        with pytest.raises(ValueError, match="max_iter must be at least 1"):
            M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=4, max_iter=it)
    for nug in (0., -1e-4, np.nan, np.inf):
        with pytest.raises(ValueError, match="the nugget must be positive"):
            M.IterativeGP._on_handle(_NoDevice(), [(0, np.ones(3), 1.1, nug, None, np.zeros(0))], 3, 9, precond_rank=4)
    v = M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=0, rtol=1e-6, max_iter=5)
    assert (v.n, v.D, v.n_emulators, v.precond_rank, v.rtol, v.max_iter) == (9, 3, 1, 0, 1e-6, 5)
    rng = np.random.default_rng(0)
    for name, call in (("V", v.matvec), ("B", v.solve)):
        for bad in (np.zeros(8), np.zeros((8, 2)), np.zeros((9, 0)), np.zeros((9, 2, 1))):
            with pytest.raises(ValueError, match="%s must have shape" % name):
                call(bad)
        b = rng.random((9, 2))
        b[3, 1] = np.nan
        with pytest.raises(ValueError, match="%s must be finite" % name):
            call(b)
        with pytest.raises(ValueError, match="emulator must be between 0 and 0"):
            call(rng.random(9), emulator=1)
    for bad in (np.zeros((4, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="testing must have shape"):
            v.predict(bad)
    q = rng.random((4, 3))
    q[0, 0] = np.inf
    with pytest.raises(ValueError, match="testing must be finite"):
        v.predict(q)
    with pytest.raises(ValueError, match="max_points must not be negative"):
        v.predict(rng.random((4, 3)), max_points=-1)
    assert _NoDevice.calls == 0
    v.close()                                     # a view leaves the handle open; afterwards it refuses by name
    with pytest.raises(RuntimeError, match="has been closed"):
        v.predict(rng.random((4, 3)))


@pytest.mark.parametrize("n,D,kernel,p", SOLVE_SHAPES, ids=lambda v: str(v))
def test_restatement_converges_within_the_cap_and_agrees_with_a_dense_solve(n, D, kernel, p):
    c, (s,) = setup(n, D, kernel)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    A = K + dc.NUGGET * np.eye(n)
    L, piv, d = ir.pivoted_cholesky(K, p) if p else (None, np.zeros(0, dtype=np.int64), None)
    B = right_hand_sides(c, s, kernel)
    sv = ir.solve(A, B, L, dc.NUGGET, RTOL, MAX_ITER)
    print("n %d D %d %s p %d: rank %d, iterations %s, residual at most %.3g" % (n, D, kernel, p, len(piv), sv.iterations.tolist(), sv.residual.max()))
    assert sv.converged.all() and sv.iterations.max() <= ITER_CAP
    if p:
        assert len(set(piv.tolist())) == len(piv) and piv[0] == 0 and np.all(d >= -1e-12)      # a constant diagonal: the first pivot is index 0
        if (n, D) == (130, 1):
            assert len(piv) < p                   # the remaining diagonal runs out: the rank stops early
    ev = np.linalg.eigvalsh(A)
    want = np.linalg.solve(A, B)
    for j in range(B.shape[1]):
        bn = np.linalg.norm(B[:, j])
        assert abs(sv.residual[j] - np.linalg.norm(B[:, j] - A @ sv.x[:, j]) / bn) <= 1e-14
        # |x - A^-1 b| <= |A^-1| |b - A x|, and what np.linalg.solve itself is off by
        bound = sv.residual[j] * bn / ev[0] + (ev[-1] / ev[0]) * n * 2. ** -52 * np.linalg.norm(want[:, j])
        assert np.linalg.norm(sv.x[:, j] - want[:, j]) <= bound


def _iterations(c, s, kernel, p, columns):
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    L = ir.pivoted_cholesky(K, p)[0]
    sv = ir.solve(K + dc.NUGGET * np.eye(K.shape[0]), np.ascontiguousarray(columns), L, dc.NUGGET, RTOL, MAX_ITER)
    assert sv.converged.all()
    return int(sv.iterations.max())


@pytest.mark.parametrize("n,D,kernel,p", PREDICT_SHAPES, ids=lambda v: str(v))
def test_restatement_converges_within_the_cap_on_every_column_the_predictions_solve(n, D, kernel, p):
    """what test_gpu_iterative.py solves beyond SOLVE_SHAPES: the weights and the 37 variance columns of the prediction tests, the residual
    of the fixed linear mean, and the three emulators (their own theta and targets, 9 queries) of the multi-output test"""
    c, (s,) = setup(n, D, kernel)
    cols = [c.T[0]] + list(ir.covariance(c.X, c.Xs, s, kernel, SIGMA2).T)
    if (n, D, kernel, p) == LINEAR_MEAN[:4]:
        cols.append(c.T[0] - (LINEAR_MEAN[4][0] + LINEAR_MEAN[4][1] * c.X[:, 0]))
    worst = _iterations(c, s, kernel, p, np.column_stack(cols))
    if (n, D, kernel, p) == MULTI[:4]:
        cm, scales_m = setup(n, D, kernel, E=MULTI[4])
        for e in range(MULTI[4]):
            cols = [cm.T[e]] + list(ir.covariance(cm.X, cm.Xs[:MULTI[5]], scales_m[e], kernel, SIGMA2).T)
            worst = max(worst, _iterations(cm, scales_m[e], kernel, p, np.column_stack(cols)))
    print("n %d D %d %s p %d: at most %d iterations over every column" % (n, D, kernel, p, worst))
    assert worst <= ITER_CAP


def test_restatement_preconditioner_cuts_the_iterations():
    c, (s,) = setup(300, 3, "SquaredExponential")
    K = ir.covariance(c.X, c.X, s, "SquaredExponential", SIGMA2)
    A = K + dc.NUGGET * np.eye(300)
    b = c.T[0][:, None]
    plain = ir.solve(A, b, None, dc.NUGGET, RTOL, MAX_ITER)
    pre = ir.solve(A, b, ir.pivoted_cholesky(K, 64)[0], dc.NUGGET, RTOL, MAX_ITER)
    assert pre.iterations[0] < 0.1 * plain.iterations[0]


def test_restatement_freezes_columns_independently():
    n, D, kernel, p = 300, 3, "Matern52", 64
    c, (s,) = setup(n, D, kernel)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    A = K + dc.NUGGET * np.eye(n)
    L = ir.pivoted_cholesky(K, p)[0]
    B = right_hand_sides(c, s, kernel)
    B[:, 3] = 0.                                  # a zero column: frozen at iteration 0 with x = 0
    block = ir.solve(A, B, L, dc.NUGGET, RTOL, MAX_ITER)
    assert block.iterations[3] == 0 and block.converged[3] and block.residual[3] == 0. and not block.x[:, 3].any()
    assert len(set(block.iterations.tolist())) > 2            # the columns do stop at different iterations
    for j in range(B.shape[1]):
        one = ir.solve(A, B[:, [j]], L, dc.NUGGET, RTOL, MAX_ITER)
        assert np.array_equal(one.x[:, 0], block.x[:, j]) and one.iterations[0] == block.iterations[j]
        assert one.residual[0] == block.residual[j] and one.converged[0] == block.converged[j]
    # a cap that is too low: not converged, x finite, the residual honest
    short = ir.solve(A, B[:, :1], L, dc.NUGGET, RTOL, 3)
    assert not short.converged[0] and short.iterations[0] == 3 and np.all(np.isfinite(short.x)) and short.residual[0] > RTOL


def test_restatement_predicts_what_the_dense_formulas_give():
    n, D, kernel = 300, 3, "SquaredExponential"
    c, (s,) = setup(n, D, kernel)
    mean, var, sa, sv = ir.predict(c.X, c.T[0], c.Xs, s, kernel, SIGMA2, dc.NUGGET, 64, RTOL, MAX_ITER)
    assert sa.converged.all() and sv.converged.all()
    A = ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET)
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    cond, amp = dc.amplification(A)
    want_mean = ks.T @ np.linalg.solve(A, c.T[0])
    want_var = np.maximum(SIGMA2 - np.sum(ks * np.linalg.solve(A, ks), axis=0) + dc.NUGGET, 0.)
    assert dc.excess("mean", mean, want_mean, amp) <= 1. and dc.excess("var", var, want_var, amp) <= 1.


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
@pytest.mark.parametrize("N,D,r,kernel", MATVEC_CASES, ids=lambda v: str(v))
def test_float64_product_lies_inside_the_bar_and_is_not_exact(N, D, r, kernel):
    c, (s,) = setup(N, D, kernel)
    V = matvec_input(N, r)
    truth = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, dtype=np.longdouble)
    got = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V)
    bar = matvec_bar(np.abs(ir.operator(c.X, s, kernel, SIGMA2, dc.NUGGET)), V, D)
    err = np.abs(np.asarray(got.astype(np.longdouble) - truth, dtype=np.float64))
    frac = float(np.max(err / bar))
    print("N %d D %d r %d %s: float64 product at %.3g of the bar" % (N, D, r, kernel, frac))
    assert 0. < frac <= 1.
    for m in dc.M_TEST:                           # the rectangular form
        cq = dc.case(N, D, kernel, m=m)
        tq = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, Q=cq.Xs, dtype=np.longdouble)
        gq = ir.matvec(c.X, s, kernel, SIGMA2, dc.NUGGET, V, Q=cq.Xs)
        bq = matvec_bar(np.abs(ir.covariance(cq.Xs, c.X, s, kernel, SIGMA2)), V, D)
        fq = float(np.max(np.abs(np.asarray(gq.astype(np.longdouble) - tq, dtype=np.float64)) / bq))
        assert 0. < fq <= 1.
