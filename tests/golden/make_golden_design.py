"""
Generate tests/golden/design.npz by IMPORTING THE REAL REFERENCE (mogp_emulator.ExperimentalDesign, mogp_emulator.SequentialDesign),
as make_golden.py does.

Runs only in the build container, never from the tests, with the reference package importable (see make_golden.py for the
environment):

    PYTHONPATH=<reference package> python -W ignore tests/golden/make_golden_design.py

The outputs are data only: seeds, inputs and the reference's outputs on them.

* ``mc_*`` / ``lhc_*``: seeded ``MonteCarloDesign`` / ``LatinHypercubeDesign`` samples.
* ``mm_*``: seeded ``MaxiMinLHC`` samples with the minimum distance of every try (captured at the reference's ``pdist`` call).  In every
  case the best and the second-best try differ by far more than the error bound of the device kernel's test, so the reference alone
  decides the winner (asserted below).
* ``mice_*``: the reference's ``MICEDesign._MICE_criterion`` of every candidate, at a FIXED theta (``gp.fit(theta)`` instead of
  ``fit_GP_MAP``: optimiser trajectories are not pinned).  Two adjustments, both as in make_golden.py section 12: ``MICEFastGP`` reads
  ``self.L``, which the refactored ``GaussianProcess`` keeps in ``self.Kinv.L`` -- the attribute is supplied; and the candidate GP gets
  the base GP's parameter VALUES (nugget = base nugget * nugget_s, the documented behaviour), not its GPParams object (which would
  silently undo nugget_s).  With nugget_s = 1 the two coincide (asserted).
  The reference forms the denominator as sigma^2 + nugget - k^T (downdated K^-1) k, a difference of two nearly equal numbers whose
  rounding error grows like 1 / nugget^2 relative to the result.  The tests compare at rtol = 1e-6, so every committed case must be one
  where the reference ITSELF is well inside that: its criterion is checked here against an evaluation in long double (64-bit
  mantissa) of the same quantity, unc1 * [K_cand^-1]_cc, and must agree to 2.5e-7 (a quarter of the tolerance).  With nugget = 1e-4
  and 400 candidates on this design the reference is 2.8e-6 from the long-double value (50 candidates: 4e-7), which is why the cases
  use 1e-3.
"""
import os

import numpy as np

import mogp_emulator.ExperimentalDesign as ED
from mogp_emulator.ExperimentalDesign import LatinHypercubeDesign, MaxiMinLHC, MonteCarloDesign
from mogp_emulator.GaussianProcess import GaussianProcess
from mogp_emulator.SequentialDesign import MICEDesign, MICEFastGP

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53


def ppf_quadratic(u):
    """A PPF the tests restate: plain float arithmetic, the same on every host."""
    return 2.0 * u * u - 1.0


# name -> constructor arguments; the tests hold the same table (callables cannot be stored)
DESIGN_ARGS = {
    "unit3": (3,),
    "box2": (2, (-1.0, 3.0)),
    "list3": ([(0.0, 1.0), (10.0, 20.0), (-5.0, -4.0)],),
    "ppf4": (4, ppf_quadratic),
    "mixed2": ([ppf_quadratic, (2.0, 2.5)],),
}

out = {}

# ---- Monte Carlo / Latin hypercube --------------------------------------------------------------------------
for cls, tag in ((MonteCarloDesign, "mc"), (LatinHypercubeDesign, "lhc")):
    for k, (name, n) in enumerate([("unit3", 7), ("box2", 1), ("list3", 20), ("ppf4", 33), ("mixed2", 12)]):
        seed = 1000 + k
        np.random.seed(seed)
        out["%s_%s_n%d_seed%d" % (tag, name, n, seed)] = cls(*DESIGN_ARGS[name]).sample(n)

# ---- maximin: samples and the minimum distance of every try -----------------------------------------------------
mm_cases = [("unit3", 10, 50, 11), ("box2", 30, 200, 12), ("list3", 65, 40, 13), ("ppf4", 129, 25, 14), ("mixed2", 2, 30, 15),
            ("unit3", 200, 1000, 16)]
real_pdist = ED.pdist
for name, n, n_tries, seed in mm_cases:
    seen = []

    def capture(X, **kw):
        d = real_pdist(X, **kw)
        seen.append(float(np.min(d)))
        return d
    ED.pdist = capture
    try:
        np.random.seed(seed)
        design = MaxiMinLHC(*DESIGN_ARGS[name])
        sample = design.sample(n, n_tries=n_tries)
    finally:
        ED.pdist = real_pdist
    seen = np.array(seen)
    assert seen.shape == (n_tries,)
    D = design.get_n_parameters()
    order = np.sort(seen)[::-1]
    bound = 2.0 * (D + 2) * EPS                                  # the relative tolerance of the device kernel's test
    assert order[0] - order[1] > 4.0 * bound * order[0], (name, order[:2])     # either value may move by `bound`: twice that, doubled
    key = "mm_%s_n%d_t%d_seed%d" % (name, n, n_tries, seed)
    out[key] = sample
    out[key + "_mins"] = seen

# ---- MICE criterion at a fixed theta -------------------------------------------------------------------------------
class PatchedFastGP(MICEFastGP):
    L = property(lambda self: self.Kinv.L)


LD = np.longdouble


def linv_longdouble(K):
    """L^-1 of K = L L^T, everything in long double."""
    n = K.shape[0]
    A = np.array(K, dtype=LD)
    for j in range(n):
        A[j, j] = np.sqrt(A[j, j] - A[j, :j] @ A[j, :j])
        if j + 1 < n:
            A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    Li = np.zeros((n, n), dtype=LD)
    for j in range(n):
        x = np.zeros(n, dtype=LD)
        x[j] = 1 / A[j, j]
        for i in range(j + 1, n):
            x[i] = -(A[i, j:i] @ x[j:i]) / A[i, i]
        Li[:, j] = x
    return Li


def sqexp_longdouble(X, Y, theta):
    D = X.shape[1]
    Xl, Yl = np.asarray(X, LD), np.asarray(Y, LD)
    e = np.exp(np.asarray(theta[:D], LD))
    r2 = sum(e[d] * (Xl[:, None, d] - Yl[None, :, d]) ** 2 for d in range(D))
    return np.exp(np.asarray(theta[D], LD)) * np.exp(-r2 / 2)


def mice_criterion_longdouble(X, C, theta, nugget, nugget_s):
    """Var_base[f(c)] / Var_cand\\c[f(c)] of every candidate; the denominator in its closed form 1 / [K_cand^-1]_cc."""
    D = X.shape[1]
    Li = linv_longdouble(sqexp_longdouble(X, X, theta) + LD(nugget) * np.eye(len(X), dtype=LD))
    v = Li @ sqexp_longdouble(C, X, theta).T
    unc1 = np.exp(LD(theta[D])) + LD(nugget) - np.sum(v * v, axis=0)
    Lc = linv_longdouble(sqexp_longdouble(C, C, theta) + LD(nugget) * LD(nugget_s) * np.eye(len(C), dtype=LD))
    return unc1 * np.sum(Lc * Lc, axis=0)


def simulator(x):
    return np.sin(3.0 * x[0]) + x[1] * x[1] - 0.5 * x[-1]


mice_cases = [("c50", 2, 40, 50, np.array([1.0, 0.3, 0.2]), 1.e-3, 1., 21),
              ("c50s", 2, 40, 50, np.array([0.5, 1.2, -0.1]), 1.e-4, 10., 22),
              ("c400", 3, 60, 400, np.array([0.8, 0.2, 1.1, 0.4]), 1.e-3, 1., 23)]
for name, D, n, n_cand, theta, nugget, nugget_s, seed in mice_cases:
    np.random.seed(seed)
    md = MICEDesign(LatinHypercubeDesign(D), n_init=n, n_cand=n_cand, nugget=nugget, nugget_s=nugget_s)
    md.generate_initial_design()
    md.set_initial_targets(np.array([simulator(x) for x in md.get_inputs()]))
    md._generate_candidates()
    # what _eval_metric does (SequentialDesign.py:937-947) with the fit replaced by a fixed theta
    md.gp = GaussianProcess(md.inputs, md.targets, nugget=md.nugget)
    md.gp.fit(theta)
    md.gp_fast = PatchedFastGP(md.candidates, np.ones(md.n_cand), nugget=md.gp.theta.nugget * md.nugget_s)
    md.gp_fast.theta = md.gp.theta.get_data()
    crit = np.array([md._MICE_criterion(i) for i in range(md.n_cand)])
    if nugget_s == 1.:
        md.gp_fast = PatchedFastGP(md.candidates, np.ones(md.n_cand), nugget=md.gp.theta.nugget * md.nugget_s)
        md.gp_fast.theta = md.gp.theta
        aliased = np.array([md._MICE_criterion(i) for i in range(md.n_cand)])
        assert np.allclose(aliased, crit, rtol=1e-12, atol=0.), name
    exact = mice_criterion_longdouble(md.inputs, md.candidates, theta, nugget, nugget_s)
    own_error = float(np.max(np.abs(crit - exact) / exact))
    print("mice %s: the reference is %.3g from the long-double value" % (name, own_error))
    assert own_error <= 2.5e-7, (name, own_error)
    top = np.sort(crit)[::-1]
    assert top[0] - top[1] > 4.e-6 * top[0], (name, top[:2])      # the test compares at rtol = 1e-6 and asks for the same argmax
    out["mice_%s_inputs" % name] = md.inputs
    out["mice_%s_targets" % name] = md.targets
    out["mice_%s_candidates" % name] = md.candidates
    out["mice_%s_theta" % name] = theta
    out["mice_%s_nugget" % name] = np.array(nugget)
    out["mice_%s_nugget_s" % name] = np.array(nugget_s)
    out["mice_%s_crit" % name] = crit
    out["mice_%s_next_target" % name] = np.array(md._estimate_next_target(md.candidates[int(np.argmax(crit))]))

path = os.path.join(HERE, "design.npz")
np.savez_compressed(path, **out)
print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
