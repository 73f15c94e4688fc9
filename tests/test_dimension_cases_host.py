"""The cases of dimension_cases.py can detect an error along D -- shown on the CPU oracle alone, before any GPU is involved.

For every D of the sweep and every kernel, at n = 130:
  * K + nugget I has a 2-norm condition number below 1e7, so the amplification max(1, cond * 1e-7) of the bars is exactly 1;
  * leaving the last input coordinate out (with its correlation parameter) moves the log-posterior, the gradient, the predictive mean and
    the variance by at least 100 x the bar test_gpu_dimension_sweep.py applies to that quantity;
  * for the kernels with one length per input, swapping the first and the last correlation parameter does the same.
The factor 100 is a condition on the inputs: a case that misses it is changed, not the factor."""
import numpy as np
import pytest

import dimension_cases as dc

QUANTITIES = ["logpost", "grad", "mean", "var"]
FACTOR = 100.


def _moved(full, other, keep=None):
    """per quantity: the largest change in units of the device test's bar"""
    g = full["grad"] if keep is None else full["grad"][keep]
    gscale = max(1., float(np.abs(full["grad"]).max()))
    out = {q: dc.excess(q, other[q], full[q]) for q in ("logpost", "mean", "var")}
    out["grad"] = dc.excess("grad", other["grad"], g, gscale=gscale)
    return out


@pytest.mark.parametrize("kernel", dc.KERNELS)
def test_cases_are_well_conditioned_and_feel_every_coordinate(kernel):
    worst_cond, least = 0., {}
    for D in dc.D_SWEEP:
        c = dc.case(dc.N_TILES, D, kernel, fit=True)
        full, ref = dc.oracle(c)
        cond, amp = dc.amplification(ref.get_K_matrix() + ref.nugget * np.eye(ref.n))
        worst_cond = max(worst_cond, cond)
        assert cond < 1e7 and amp == 1., (kernel, D, cond)
        if D < 2:
            continue
        per_dim = kernel in dc.PER_DIM
        theta = c.thetas[0]
        keep = np.delete(np.arange(theta.size), D - 1) if per_dim else np.arange(theta.size)
        moves = {"drop": _moved(full, dc.oracle(c, X=c.X[:, :-1], Xs=c.Xs[:, :-1], theta=theta[keep])[0], keep)}
        if per_dim:
            sw = theta.copy()
            sw[0], sw[D - 1] = theta[D - 1], theta[0]
            other = dc.oracle(c, theta=sw)[0]
            other["grad"] = other["grad"].copy()
            other["grad"][[0, D - 1]] = other["grad"][[D - 1, 0]]          # the entry of each parameter, in the full case's order
            moves["swap"] = _moved(full, other)
        for what, mv in moves.items():
            for q in QUANTITIES:
                least[(what, q)] = min(least.get((what, q), np.inf), mv[q])
                assert mv[q] >= FACTOR, (kernel, D, what, q, mv[q])
    print("%s: largest cond %.3g; smallest change in units of the bar: %s" % (
        kernel, worst_cond, ", ".join("%s %s %.3g" % (w, q, v) for (w, q), v in sorted(least.items()))))
