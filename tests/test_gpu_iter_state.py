"""The cached state of the iterative solver (csrc/iter_solver.h) across a SEQUENCE of calls on one handle: the preconditioner and its key,
the variance cache and its key, the kept alpha per emulator, and the scaled design the handle re-forms when other scales come.  Every other
GPU test of the unit uses a fresh handle or repeats one call; a state refactor can break exactly what lies between two different calls.

Each case walks a handle through its calls, ends with one call on that handle and the same call on a FRESH handle, and compares every
output as bytes: nothing that an earlier call left behind may reach a result.  The calls go through LibGPGPU.LocalGP_GPU, the thinnest
Python entry that reaches the mogp_local_* C entries.

Shapes: N = 130 (three row tiles, the last partly filled), D = 1 and 3, both kernels, ranks 32 and 64, two residual rows, 37 queries,
rtol 1e-8 -- the smallest at which a panel has a partly filled block and the pivoted factor can stop early (D = 1).  Designs, targets,
hyperparameters (theta_1, theta_2: those of emulators 0 and 1 of dimension_cases.case) and right-hand sides are those of
test_iterative_host.py, the probes those of large_design_cases.apply_probes.

The two key drops of the groups' reserve can only be seen where a call is refused AFTER it grew a buffer and BEFORE it built into it: a
call that completes always builds for its own key, which holds the rank and therefore differs from the key of the smaller buffer.  Cases
7 and 8 do that with max_points = -1, which predict_plan.h refuses behind the reservation."""
import functools

import numpy as np
import pytest

from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.LocalGP import _KERNELS

import dimension_cases as dc
import large_design_cases as ld
import test_iterative_host as th
from test_iterative_host import MAX_ITER, SIGMA2

pytestmark = pytest.mark.gpu

N, E, M_Q, RTOL = 130, 2, dc.M_TEST[0], 1e-8
P1, P2 = 32, 64
SHAPES = [(D, kernel) for D in (1, 3) for kernel in ("SquaredExponential", "Matern52")]
shapes = pytest.mark.parametrize("D,kernel", SHAPES, ids=lambda v: str(v))


class _Setup(object):
    """the inputs of one shape, computed once and never changed, and the calls with the hyperparameters filled in"""

    def __init__(self, D, kernel):
        self.c, (self.s1, self.s2) = th.setup(N, D, kernel, m=M_Q, E=E)
        assert not np.array_equal(self.s1, self.s2)
        self.kt = _KERNELS[kernel][0]
        self.B = th.right_hand_sides(self.c, self.s1, kernel)             # (N, 8)
        self.V = th.matvec_input(N, 3)
        for a in (self.c.X, self.c.T, self.c.Xs, self.s1, self.s2, self.B, self.V):
            a.setflags(write=False)

    def handle(self):
        return LibGPGPU.LocalGP_GPU(self.c.X, self.c.T)

    def hyper(self, s):
        return (self.kt, s, SIGMA2, dc.NUGGET)

    def precondition(self, h, s, p):
        return h.precondition(*self.hyper(s), p)[0]

    def solve(self, h):
        return h.solve(self.B, RTOL, MAX_ITER)

    def bound(self, h, s, p, **kw):
        return h.variance_bound(*self.hyper(s), p, True, self.c.Xs, return_cache=True, **kw)

    def predict(self, h, e, rtol=RTOL, p=P1, unc=False, **kw):
        return h.predict_exact(e, *self.hyper(self.s1), p, rtol, MAX_ITER, True, self.c.Xs, unc=unc, return_alpha=True, **kw)

    def loglik(self, h, g1, g2):
        return h.loglik_exact(0, *self.hyper(self.s1), P1, RTOL, MAX_ITER, g1, g2, grad=True, probe_terms=True, return_panels=True)


@functools.lru_cache(maxsize=None)
def _setup(D, kernel):
    return _Setup(D, kernel)


def _bits(x):
    """every array of a result as bytes, whatever its nesting"""
    if x is None:
        return None
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in sorted(x.items())}
    if isinstance(x, (tuple, list)):
        return [_bits(v) for v in x]
    return np.ascontiguousarray(x).tobytes()


def _same(used, fresh):
    assert _bits(used) == _bits(fresh)


def _probes(u, reached):
    name, g1, g2 = ld.apply_probes(N, reached)[1]
    assert name == "dense"
    return g1, g2


def _rank_reached(u):
    h = u.handle()
    r = u.precondition(h, u.s1, P1)
    h.close()
    return r


@shapes
def test_solve_after_the_scaled_design_was_formed_for_other_scales(D, kernel):
    """1. precondition(theta_1, 32); kmatvec at the scales of theta_2; solve"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    u.precondition(h, u.s1, P1)
    h.kmatvec(*u.hyper(u.s2), u.V)
    used = u.solve(h)
    u.precondition(f, u.s1, P1)
    fresh = u.solve(f)
    h.close(), f.close()
    assert used[2].all()
    _same(used, fresh)


@shapes
def test_variance_cache_outlives_a_preconditioner_of_other_hyperparameters(D, kernel):
    """2. variance_bound(theta_1, 32); precondition(theta_2, 64): the factor's buffer grows; variance_bound(theta_1, 32) again"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    first = u.bound(h, u.s1, P1)
    u.precondition(h, u.s2, P2)
    used = u.bound(h, u.s1, P1)
    fresh = u.bound(f, u.s1, P1)
    h.close(), f.close()
    assert used[1] >= 1
    _same(first, fresh)
    _same(used, fresh)


@shapes
def test_variance_cache_after_its_own_buffers_grew(D, kernel):
    """3. variance_bound(theta_1, 32); variance_bound(theta_1, 64): the cache's buffers grow; variance_bound(theta_1, 32)"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    u.bound(h, u.s1, P1)
    u.bound(h, u.s1, P2)
    used = u.bound(h, u.s1, P1)
    fresh = u.bound(f, u.s1, P1)
    h.close(), f.close()
    _same(used, fresh)


@shapes
def test_likelihood_replaces_the_kept_alpha_of_its_emulator_alone(D, kernel):
    """4. predict_exact(e = 0); loglik_exact(e = 0) with the same key; predict_exact(e = 0) without the variance; then predict_exact(e = 1)"""
    u = _setup(D, kernel)
    g1, g2 = _probes(u, _rank_reached(u))
    h, f = u.handle(), u.handle()
    u.predict(h, 0, unc=True)
    u.loglik(h, g1, g2)
    used = u.predict(h, 0)
    fresh = u.predict(f, 0)
    assert used[2][1] and used[1] is None
    _same(used, fresh)                                         # mean, the three statistics, alpha
    used1, fresh1 = u.predict(h, 1), u.predict(f, 1)
    h.close(), f.close()
    _same(used1, fresh1)
    assert not np.array_equal(used1[4], used[4])


@shapes
def test_another_rtol_solves_alpha_again(D, kernel):
    """5. predict_exact at rtol 1e-8, then at 1e-4: the statistics are those of a fresh handle at 1e-4, not the kept ones"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    tight = u.predict(h, 0)
    used = u.predict(h, 0, rtol=1e-4)
    fresh = u.predict(f, 0, rtol=1e-4)
    h.close(), f.close()
    print("D %d %s: alpha solve (iterations, converged, residual) at rtol 1e-8 %s, at 1e-4 %s" % (D, kernel, tight[2], used[2]))
    _same(used, fresh)


@shapes
def test_a_call_refused_after_the_preconditioner_was_built(D, kernel):
    """6. loglik_exact with g1 one row short of the rank reached is refused behind the build; then the valid call"""
    u = _setup(D, kernel)
    reached = _rank_reached(u)
    g1, g2 = _probes(u, reached)
    h, f = u.handle(), u.handle()
    with pytest.raises(RuntimeError, match="loglik_exact: g1 must have as many rows as the rank the preconditioner reaches, %d" % reached):
        u.loglik(h, g1[:-1], g2)
    used = u.loglik(h, g1, g2)
    fresh = u.loglik(f, g1, g2)
    h.close(), f.close()
    assert used["rank"] == reached and used["converged"].all()
    _same(used, fresh)


@shapes
def test_a_refusal_behind_a_grown_factor_leaves_no_preconditioner(D, kernel):
    """7. precondition(theta_1, 32); predict_exact at rank 64 refused behind the reservation: the factor's buffer grew and nothing was built
    into it, so solve is refused as on a fresh handle; then precondition(theta_1, 32) and solve"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    u.precondition(h, u.s1, P1)
    with pytest.raises(RuntimeError, match="predict_exact: max_points must not be negative"):
        u.predict(h, 0, p=P2, max_points=-1)
    for handle in (h, f):
        with pytest.raises(RuntimeError, match="solve: precondition has not been called"):
            u.solve(handle)
    u.precondition(h, u.s1, P1)
    used = u.solve(h)
    u.precondition(f, u.s1, P1)
    fresh = u.solve(f)
    h.close(), f.close()
    _same(used, fresh)


@shapes
def test_a_refusal_behind_a_grown_variance_cache_leaves_no_cache(D, kernel):
    """8. variance_bound(theta_1, 32); variance_bound(theta_1, 64) refused behind the reservation: the cache's buffers grew and nothing was
    built into them; variance_bound(theta_1, 32) builds again"""
    u = _setup(D, kernel)
    h, f = u.handle(), u.handle()
    u.bound(h, u.s1, P1)
    with pytest.raises(RuntimeError, match="variance_bound: max_points must not be negative"):
        u.bound(h, u.s1, P2, max_points=-1)
    used = u.bound(h, u.s1, P1)
    fresh = u.bound(f, u.s1, P1)
    h.close(), f.close()
    _same(used, fresh)
