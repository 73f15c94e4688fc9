"""Host-side checks of the variance bound (mogp_emulator_amd.IterativeGP variance_bound / variance_cache / predict(unc="bound")):

* the NumPy restatement (variance_bound_restate.py) against the dense predictive variance on every shape the GPU tests use: the bound is
  never below it, equals it at rank N, is non-increasing in the rank bit for bit, and the cache's rank stops below the preconditioner's where
  the columns of L run into rounding noise;
* the restatement against itself on a matrix rounded another way: the bound is determined to its bar on every shape, the columns of R
  wherever no prefix is cut -- and NOT the last columns a cut keeps (reference_own_error: the columns a device result is held to);
* the bytes, the memory refusal and the refusal texts of csrc/predict_plan.h (tests/c/iter_var_plan_check.cpp) and the prefix Cholesky and
  triangular product of csrc/iter_var_host.h (tests/c/iter_var_host_check.cpp), as sanitised stand-alone programs;
* the Python refusals, which come before any device call, and the exports.

SHAPES and the bar are defined here and imported by test_gpu_variance_bound.py.  The bar is that of the variance everywhere else in the
suite, dc.BARS["var"] at the scale sigma^2, multiplied by the amplification of the matrix that is factorised last, H = Q^T A Q."""
import importlib
import os

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

import dimension_cases as dc
import iterative_restate as ir
import test_iterative_host as th
import variance_bound_restate as vr
from test_iterative_host import SIGMA2

IG = importlib.import_module("mogp_emulator_amd.IterativeGP")
ROOT = th.ROOT
M_Q = dc.M_TEST[-1]

FULL_RANK = [(130, 17, "SquaredExponential", 130), (130, 3, "Matern52", 130), (300, 3, "UniformMat52", 300)]
EARLY_STOP = [(130, 1, "SquaredExponential", 32), (300, 1, "UniformSqExp", 64)]      # var_rank < the rank the preconditioner reaches
SHAPES = [s for s in th.SOLVE_SHAPES if s[3] > 0] + FULL_RANK + [(130, 1, "Matern52", 64), (300, 1, "UniformSqExp", 64)]


def slack(H):
    """the absolute bar of a variance at the scale sigma^2, amplified by cond(H)"""
    rtol, atol = dc.BARS["var"]
    cond, amp = dc.amplification(H)
    return amp * (atol + rtol * SIGMA2), cond, amp


def column_excess(R, want, amp):
    """dc.excess("fullcov", ., ., amp) column by column"""
    return np.array([dc.excess("fullcov", R[:, j], want[:, j], amp) for j in range(want.shape[1])])


def reference_own_error(c, s, kernel, ch, amp):
    """Per column of the restatement's R: its excess over the "fullcov" bar against the restatement of the SAME matrix rounded another way
    (K evaluated in long double and rounded once: entries that differ by an ulp or two), on the same pivots.  Where the first prefix is cut
    by tau the last columns it keeps are what is left of a column of L after the ones before it are projected out -- a difference of nearly
    equal vectors -- and no float64 computation determines them to the bar: there this figure is above 1 for the restatement itself, and
    a column-wise comparison of a device result with it says nothing (the subspace's bound and R^T A R = I are checked instead)."""
    K2 = np.asarray(ir.covariance(c.X, c.X, s, kernel, SIGMA2, dtype=np.longdouble), dtype=np.float64)
    other = vr.cache(K2, dc.NUGGET, ch.L.shape[1], pivots=ch.pivots)
    r = min(ch.var_rank, other.var_rank)
    own = np.full(ch.var_rank, np.inf)
    own[:r] = column_excess(other.R[:, :r], ch.R[:, :r], amp)
    return own


@pytest.mark.parametrize("n,D,kernel,p", SHAPES, ids=lambda v: str(v))
def test_restatement_determines_the_bound_everywhere_and_its_columns_away_from_the_cut(n, D, kernel, p):
    """the restatement against itself on a matrix that differs by an ulp or two per entry: which of its columns a device result can be
    held to (test_gpu_variance_bound.py takes them from reference_own_error), and that the BOUND is determined to its bar on every shape"""
    c, (s,) = th.setup(n, D, kernel, m=M_Q)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    ch = vr.cache(K, dc.NUGGET, p)
    bar, cond, amp = slack(ch.H)
    own = reference_own_error(c, s, kernel, ch, amp)
    K2 = np.asarray(ir.covariance(c.X, c.X, s, kernel, SIGMA2, dtype=np.longdouble), dtype=np.float64)
    other = vr.cache(K2, dc.NUGGET, ch.L.shape[1], pivots=ch.pivots)
    e_b = dc.excess("var", vr.bound(other.R, ks, SIGMA2, dc.NUGGET), vr.bound(ch.R, ks, SIGMA2, dc.NUGGET), amp)
    print("n %d D %d %s p %d: var_rank %d / %d, columns of R determined to the bar: %d of %d (largest own error %.3g bars, at column %d); "
          "the bound differs by %.3g of its bar" % (n, D, kernel, p, ch.var_rank, other.var_rank, int(np.count_nonzero(own <= 1.)), ch.var_rank,
                                                    own.max(), int(np.argmax(own)), e_b))
    assert other.var_rank == ch.var_rank and e_b <= 1.
    if ch.var_rank == ch.L.shape[1]:
        assert np.all(own <= 1.)                               # no cut: every column is determined


@pytest.mark.parametrize("n,D,kernel,p", SHAPES, ids=lambda v: str(v))
def test_restatement_bounds_the_dense_variance(n, D, kernel, p):
    c, (s,) = th.setup(n, D, kernel, m=M_Q)
    K = ir.covariance(c.X, c.X, s, kernel, SIGMA2)
    A = K + dc.NUGGET * np.eye(n)
    ks = ir.covariance(c.X, c.Xs, s, kernel, SIGMA2)
    ch = vr.cache(K, dc.NUGGET, p)
    reached = ch.L.shape[1]
    bar, cond, amp = slack(ch.H)
    dense = vr.dense_variance(A, ks, SIGMA2, dc.NUGGET)
    prof = vr.profile(ch.R, ks, SIGMA2, dc.NUGGET)
    got = vr.bound(ch.R, ks, SIGMA2, dc.NUGGET)
    gap = got - dense
    ortho = float(np.max(np.abs(ch.Q.T @ ch.Q - np.eye(ch.r0)))) if ch.r0 else 0.
    unit = float(np.max(np.abs(ch.R.T @ A @ ch.R - np.eye(ch.var_rank)))) if ch.var_rank else 0.
    print("n %d D %d %s p %d: rank reached %d, r0 %d, var_rank %d, cond(H) %.3g, Q^T Q - I %.3g, R^T A R - I %.3g, (bound - dense) / sigma^2 "
          "mean %.3g max %.3g min %.3g (bar %.3g)" % (n, D, kernel, p, reached, ch.r0, ch.var_rank, cond, ortho, unit, gap.mean() / SIGMA2,
                                                      gap.max() / SIGMA2, gap.min() / SIGMA2, bar / SIGMA2))
    assert 1 <= ch.var_rank <= ch.r0 <= reached <= p
    assert np.array_equal(got, prof[ch.var_rank]) and np.all(np.isfinite(prof))
    assert np.all(got >= dense - bar)                                            # never over-confident
    assert np.all(prof[1:] <= prof[:-1])                                         # tightens with the rank, exactly
    for r in (1, ch.var_rank // 2, ch.var_rank):                                 # nested: the leading columns are the cache of that rank
        if r >= 1:
            small = vr.cache(K, dc.NUGGET, r, pivots=ch.pivots)
            assert small.var_rank == r
            assert np.max(np.abs(vr.bound(small.R, ks, SIGMA2, dc.NUGGET) - prof[r])) <= bar
    if (n, D, kernel, p) in FULL_RANK:
        assert ch.var_rank == n and np.max(np.abs(gap)) <= bar                   # the exact variance at rank N
    if (n, D, kernel, p) in EARLY_STOP:
        assert ch.var_rank < reached
    no_nugget = vr.bound(ch.R, ks, SIGMA2, dc.NUGGET, include_nugget=False)
    assert np.all(no_nugget <= got) and np.all(no_nugget >= vr.dense_variance(A, ks, SIGMA2, dc.NUGGET, include_nugget=False) - bar)


def test_prefix_cholesky_of_the_restatement_stops_and_is_a_prefix():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 6))
    B[:, 4] = B[:, 0] - 2. * B[:, 2]                       # column 4 depends on the columns before it
    G = B.T @ B
    C, r = vr.prefix_cholesky(G, vr.TAU * G[0, 0])
    assert r == 4 and np.allclose(C @ C.T, G[:4, :4], rtol=1e-12, atol=1e-12)
    C3, r3 = vr.prefix_cholesky(G[:3, :3], 0.)
    assert r3 == 3 and np.array_equal(C3, C[:3, :3])
    U = vr.inverse_transposed(C)
    assert np.allclose(U, np.linalg.inv(C).T, rtol=1e-12, atol=1e-12) and np.array_equal(U, np.triu(U))
    Q = B[:, :4] @ U
    assert np.max(np.abs(Q.T @ Q - np.eye(4))) <= 1e-13


def test_plan_bytes_memory_refusal_and_refusal_texts(tmp_path):
    out = th._build_and_run(tmp_path, "iter_var_plan_check")
    assert out.strip() == "ok 21 checks"


def test_host_prefix_cholesky_and_triangular_product(tmp_path):
    out = th._build_and_run(tmp_path, "iter_var_host_check")
    assert out.strip() == "ok 9 checks"


def test_exports():
    assert IG.IterativeGP.VAR_CHUNK == IG.VAR_CHUNK == 64
    for name in ("variance_bound", "variance_cache", "variance_gap"):
        assert callable(getattr(M.IterativeGP, name))
    assert "variance_bound" in M.__doc__
    p = M.IterativePrediction(1, 2, 3, 4, 5, 6, 7)                                # the earlier construction still works
    assert (p.var_rank, p.unc_kind) == (None, "exact") and M.IterativePrediction(1, None, 3, 4, 5, None, None).unc_kind is None
    header = open(os.path.join(ROOT, "include", "mogp_hip.h")).read()
    assert "mogp_local_variance_bound(" in header
    plan = open(os.path.join(ROOT, "mogp_emulator_amd", "csrc", "predict_plan.h")).read()
    assert "ITER_VAR_CHUNK = %d" % IG.VAR_CHUNK in plan
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        assert "mogp_local_variance_bound" in _capi.SIGNATURES and len(_capi.SIGNATURES["mogp_local_variance_bound"][1]) == 15
        assert hasattr(LibGPGPU.LocalGP_GPU, "variance_bound")


class _NoDevice(object):
    """stands for the native handle; anything that would go to the device is an error"""
    calls = 0

    def _touch(self, *a, **k):
        _NoDevice.calls += 1
        raise AssertionError("the device must not be reached")

    kmatvec = precondition = solve = predict_exact = variance_bound = _touch

    def close(self):
        pass


def test_refusals_come_before_any_device_call():
    good = [(0, np.ones(3), 1.1, 1e-4, None, np.zeros(0))]
    rng = np.random.default_rng(0)
    q = rng.random((4, 3))
    v = M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=4)
    for bad in ("Bound", "exact", "", "true", "bounds"):
        with pytest.raises(ValueError, match='IterativeGP.predict: unc must be False, True or "bound"'):
            v.predict(q, unc=bad)
    for bad in (0, -1, 5, 2.5):
        with pytest.raises(ValueError, match="IterativeGP.variance_bound: rank must be between 1 and precond_rank = 4"):
            v.variance_bound(q, rank=bad)
    for bad in (np.zeros((4, 2)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="IterativeGP.variance_bound: testing must have shape"):
            v.variance_bound(bad)
        with pytest.raises(ValueError, match="IterativeGP.variance_gap: testing must have shape"):
            v.variance_gap(bad)
    with pytest.raises(ValueError, match="IterativeGP.variance_bound: max_points must not be negative"):
        v.variance_bound(q, max_points=-1)
    for call in (lambda: v.variance_bound(q, emulator=1), lambda: v.variance_cache(emulator=1), lambda: v.variance_gap(q, emulator=1)):
        with pytest.raises(ValueError, match="emulator must be between 0 and 0"):
            call()
    plain = M.IterativeGP._on_handle(_NoDevice(), good, 3, 9, precond_rank=0)
    for who, call in (("predict", lambda: plain.predict(q, unc="bound")), ("variance_bound", lambda: plain.variance_bound(q)),
                      ("variance_cache", lambda: plain.variance_cache()), ("variance_gap", lambda: plain.variance_gap(q))):
        with pytest.raises(ValueError, match="IterativeGP.%s: the variance bound is built from the preconditioner's factor: precond_rank must be "
                                             "at least 1" % who):
            call()
    assert _NoDevice.calls == 0
    v.close()
    for call in (lambda: v.variance_bound(q), lambda: v.variance_cache(), lambda: v.variance_gap(q), lambda: v.predict(q, unc="bound")):
        with pytest.raises(RuntimeError, match="has been closed"):
            call()
    assert _NoDevice.calls == 0
