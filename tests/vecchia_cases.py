"""The shapes of the Vecchia tests (test_vecchia_host.py, test_gpu_vecchia.py) and their restatement values, computed once per process and
shared.  Inputs come from dimension_cases.case (its theta rule and NUGGET); plain NumPy, nothing here touches the device.

Everything the restatement (vecchia_restate.py) computes is in the VECCHIA ORDER (row p of X[order]); the class under test speaks the
caller's numbering.  to_caller / to_positions translate neighbour lists, and rows of per-point arrays move with out[order] = in."""
import functools

import numpy as np

import dimension_cases as dc
import local_cases as lc
import local_restate as lr
import vecchia_restate as vr

KERNELS = lc.KERNELS
ORDERS = ["identity", "reversed", "random"]
NEIGHBOUR_SHAPES = [(130, 3, 8), (300, 3, 50), (127, 2, 126), (130, 17, 126), (1000, 5, 64)]       # (N, D, k)
NEIGHBOUR_SWEEP_D = [1, 16, 17, 33, 80]                                                           # at N = 130, k = 16
# (N, D, k, kernel, nugget fitted): k below and above one wave of the best list with every kernel and both nugget modes, and the tile's limit
VALUE_CASES = [(N, D, k, kern, fit) for kern in KERNELS for fit in (True, False) for (N, D, k) in ((130, 3, 8), (300, 3, 50))] + [
    (130, 17, 126, "SquaredExponential", True), (130, 17, 126, "Matern52", False)]
LIMIT = (127, 2, 126)                                                                              # k = N - 1: the exact likelihood
SIGMA2 = lc.SIGMA2


def order_of(name, N):
    if name == "identity":
        return np.arange(N)
    if name == "reversed":
        return np.arange(N)[::-1].copy()
    return np.random.default_rng([7, N]).permutation(N)


def to_caller(nbr_pos, order):
    """lists in positions of the Vecchia order -> (N, k) in the caller's numbering, row i = the list of point i"""
    out = np.empty_like(nbr_pos)
    out[order] = np.where(nbr_pos >= 0, order[np.maximum(nbr_pos, 0)], -1)
    return out


def to_positions(nbr_caller, order):
    """the inverse of to_caller"""
    pos = np.empty_like(order)
    pos[order] = np.arange(order.shape[0])
    rows = nbr_caller[order]
    return np.where(rows >= 0, pos[np.maximum(rows, 0)], -1)


@functools.lru_cache(maxsize=None)
def setup(N, D, kernel, fit):
    """(case, theta, s, sigma^2, nugget)"""
    c = dc.case(N, D, kernel, fit=fit)
    theta = c.thetas[0]
    s, sigma2, nugget = vr.unpack(theta, D, kernel, "fit" if fit else dc.NUGGET)
    return c, theta, s, sigma2, nugget


@functools.lru_cache(maxsize=None)
def neighbours(N, D, k, kernel, order_name):
    """(order, the restatement's lists in positions, the same in the caller's numbering)"""
    c, theta, s, _, _ = setup(N, D, kernel, False)
    order = order_of(order_name, N)
    pos = vr.ordered_neighbours(c.X[order], s, k)
    return order, pos, to_caller(pos, order)


@functools.lru_cache(maxsize=None)
def reference(N, D, k, kernel, fit, order_name="random"):
    """the restatement on its own lists, float64: dict(order, nbr (positions), terms, grad rows, cond), all in the Vecchia order"""
    c, theta, s, sigma2, nugget = setup(N, D, kernel, fit)
    order, pos, _ = neighbours(N, D, k, kernel, order_name)
    terms, g, ok, cond = vr.terms(c.X[order], c.T[0][order], s, kernel, sigma2, nugget, pos, grad=True, fit_nugget=fit)
    assert ok.all()
    return dict(order=order, nbr=pos, terms=terms, grad=g, cond=cond)


def excess_rows(tag, got, want, cond):
    return lc.excess_rows(tag, got, want, cond)
