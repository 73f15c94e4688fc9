"""The replica engine of fit_GP_MAP (Engine::fit_map): its slots take the runs of whatever emulator comes next (Engine::retarget), and
the engine of the last multi-start fit of a process is kept and taken again by the next fit of the same shape (MOGP_REPLICA_CACHE).
Both hand-overs must leave nothing of the previous owner behind: not its design matrix H(X) of an analytic mean, not its
pivot-ordered copy of the inputs.  Either would leave the optimiser on a wrong objective with a plausible, finite answer.

The cache is process-wide, so every scenario runs in fresh child processes, one after the other.  Each is checked three ways:
  * against the same script on a fresh engine (MOGP_REPLICA_CACHE=0), bit for bit -- or, where runs of different emulators share
    slots, against one slot per emulator (MOGP_PARALLEL_STARTS=0);
  * against the oracle, independently of the library: the log-posterior at the device's theta, and that theta is a stationary point
    of the true objective (small oracle gradient, nothing left for an L-BFGS-B polish on the oracle);
  * by the diagnostic counters: the fit really took the cached engine, slots were retargeted, pivot-ordered inputs were restored."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose
from scipy.optimize import minimize

from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_OPTIONS = dict(max_iter=200, ftol=1e-12, gtol=1e-8)
CORR_PRIOR, COV_PRIOR, NUG_PRIOR = (3., 1.), (3., 2.), (2., 1e-3)      # InvGamma (shape, scale)
# Stationarity bounds on the oracle objective at the device's optimum (log-posteriors of -100 to -700 here).  With the optimiser
# options above the largest oracle gradient entry over all scenarios was 1.8e-4 and an L-BFGS-B polish gained at most 5e-11; the
# bounds leave a factor of 25 on the gradient and 2e4 on the gain.  Runs on a wrong objective ended with gradients of 1.5 - 100 and
# polish gains of 0.25 - 670.
GRAD_BOUND = 5e-3
POLISH_BOUND = 1e-6


def make_data(seed, n, D, n_out, repeats=0):
    """Inputs in [0, 1]^D and smooth targets with a linear trend (the analytic mean has something to fit).  The targets are functions
    of the inputs alone, so repeated design points (the last `repeats` rows copy the first ones) carry equal targets."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, D))
    if repeats:
        X[n - repeats:] = X[:repeats]
    W = rng.normal(size=(n_out, D))
    T = np.stack([1. + 0.5 * k + 2. * X[:, 0] - 1.5 * X[:, 1] + np.sin(3. * X @ W[k]) + 0.02 * np.sin(40. * X @ W[k] + k)
                  for k in range(n_out)])
    return X, T


def priors(D, nugget_type):
    from mogp_emulator_amd.Priors import GPPriors, InvGammaPrior
    return GPPriors(corr=[InvGammaPrior(*CORR_PRIOR) for _ in range(D)], cov=InvGammaPrior(*COV_PRIOR),
                    nugget=InvGammaPrior(*NUG_PRIOR) if nugget_type == "fit" else None, nugget_type=nugget_type)


def nugget_kind(nugget):
    return "fixed" if isinstance(nugget, float) else nugget


# One child process: a sequence of multi-start fits, the last one reported.  A fit is a dict:
#   seed: data seed (same n, D, outputs in every fit of the sequence), nugget: "fit" / "adaptive" / "pivot" / float,
#   terms: analytic mean terms (None: zero mean), n_tries, multi: MultiOutputGP (else GaussianProcessGPU on output 0),
#   switch: {emulator: nugget} set on the native emulators after construction, repeats: repeated design points.
_CHILD = r"""
import ctypes, json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, _capi
from test_gpu_replica import make_data, priors, nugget_kind, FIT_OPTIONS
spec = json.loads(%(spec)r)
lib = _capi.load()

def counter(name):
    c = ctypes.c_longlong(-1)
    return c.value if lib.mogp_profile_counter(name.encode(), ctypes.byref(c)) == 0 else None

LibGPGPU.set_fit_options(seed=spec["opt_seed"], **FIT_OPTIONS)
names = ("retargets", "replica_engines_reused", "replica_inputs_restored")
for fit in spec["fits"]:
    X, T = make_data(fit["seed"], spec["n"], spec["D"], spec["n_out"], fit.get("repeats", 0))
    kw = dict(kernel=spec["kernel"], nugget=fit["nugget"], priors=priors(spec["D"], nugget_kind(fit["nugget"])))
    if fit.get("terms"):
        kw.update(mean=LibGPGPU.PolyMeanFunc(fit["terms"]), analytic_mean=True)
    if fit.get("multi"):
        gp = M.MultiOutputGP_GPU(X, T, **kw)
        for i, nug in fit.get("switch", {}).items():
            em = gp._mogp_gpu.emulator(int(i))
            em.set_nugget_type(getattr(LibGPGPU.nugget_type, nugget_kind(nug)))
            if isinstance(nug, float):
                em.set_nugget_size(nug)
    else:
        gp = M.GaussianProcessGPU(X, T[0], **kw)
    before = {k: counter(k) for k in names}
    gp = M.fit_GP_MAP(gp, n_tries=fit["n_tries"])
    after = {k: counter(k) for k in names}
ems = gp.emulators if fit.get("multi") else [gp]
assert all(em.theta.data_has_been_set() for em in ems)
out = {"theta": [list(map(float, em.theta.get_data())) for em in ems],
       "logpost": [float(em.current_logpost) for em in ems],
       "nugget": [str(em._densegp_gpu.get_nugget_type()).split(".")[1] for em in ems],
       "rank": [int(em.pivot_rank) for em in ems],
       "grad": [list(map(float, em.logpost_deriv(em.theta.get_data()))) for em in ems],
       "last_fit": {k: (None if after[k] is None else after[k] - before[k]) for k in names},
       "process": {k: counter(k) for k in names}}
print("REPLICA-RESULT " + json.dumps(out))
"""


def run_child(spec, env):
    script = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "spec": json.dumps(spec)}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "REPLICA-RESULT" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.split("REPLICA-RESULT ")[1].splitlines()[0])


def oracle_for(spec, k):
    fit = spec["fits"][-1]
    X, T = make_data(fit["seed"], spec["n"], spec["D"], spec["n_out"], fit.get("repeats", 0))
    nug = fit.get("switch", {}).get(str(k), fit["nugget"])
    kind = nugget_kind(nug)
    D = spec["D"]
    rpri = R.GPPriorsRef(D, kind, corr=[R.Prior("invgamma", *CORR_PRIOR) for _ in range(D)], cov=R.Prior("invgamma", *COV_PRIOR),
                         nugget=R.Prior("invgamma", *NUG_PRIOR) if kind == "fit" else None)
    kw = dict(kernel=spec["kernel"], nugget=nug, priors=rpri)
    if fit.get("terms"):
        return R.GPRefMean(X, T[k], [tuple(t) for t in fit["terms"]], True, **kw), kind
    return R.GPRef(X, T[k], **kw), kind


def objective(ref, lp):
    # (a trial point of the polish where the oracle has no finite value -- K not positive definite with a fixed nugget, a pivoted
    # factor with underflowing replacement diagonal -- counts as no improvement)
    def f(theta):
        with np.errstate(all="ignore"):
            try:
                v, g = ref.logposterior(theta), ref.logpost_deriv(theta)
            except (np.linalg.LinAlgError, ValueError, FloatingPointError):
                v, g = np.inf, None
        if not np.isfinite(v) or not np.all(np.isfinite(g)):
            return abs(lp) + 1e10, np.zeros_like(theta)
        return v, g
    return f


def check_oracle(spec, res):
    """The device's log-posterior and gradient at its theta are the oracle's, and that theta is a stationary point of the oracle
    objective.  A pivoted emulator whose factor skips pivots beyond the first 64 columns is held to its log-posterior only, at 1e-4:
    there the value carries rounding residue of the skipped block amplified by replacement diagonals, whose size depends on how the
    LAPACK build blocks dpstrf (test_gpu_pivot.py::test_two_repeated_points_beyond_one_block_keep_lapacks_blocked_tail; 2.9e-6 measured
    here), and the objective jumps where the rank changes, so an end point on such an edge is no stationary point.  The parity of the
    calling test covers those emulators tightly."""
    for k, (theta, lp) in enumerate(zip(res["theta"], res["logpost"])):
        ref, kind = oracle_for(spec, k)
        assert res["nugget"][k] == kind
        theta = np.array(theta)
        deficient = kind == "pivot" and res["rank"][k] < ref.n
        assert_allclose(lp, ref.fit(theta), rtol=1e-4 if deficient else 1e-8, err_msg="emulator %d: log-posterior at the device's theta" % k)
        if deficient:
            continue
        assert_allclose(res["grad"][k], ref.logpost_deriv(theta), rtol=1e-5, atol=1e-5, err_msg="emulator %d: gradient" % k)
        g = np.abs(ref.logpost_deriv(theta)).max()
        pol = minimize(objective(ref, lp), theta, jac=True, method="L-BFGS-B", options=dict(maxiter=200, ftol=1e-15, gtol=1e-10))
        gain = lp - pol.fun
        print("emulator %d (%s): logpost %.10g, max |oracle grad| %.3g, polish gain %.3g" % (k, kind, lp, g, gain))
        assert g < GRAD_BOUND, "emulator %d: oracle gradient %.3g at the device's optimum" % (k, g)
        assert gain < POLISH_BOUND, "emulator %d: an oracle polish improves the log-posterior by %.3g" % (k, gain)


def spec_of(fits, n=200, D=3, n_out=1, kernel="SquaredExponential", opt_seed=7):
    return dict(fits=fits, n=n, D=D, n_out=n_out, kernel=kernel, opt_seed=opt_seed)


def check_reuse(spec, restored=False):
    """Scenarios A, B, D: the last fit takes the cached replica engine; a fresh engine ends at the same point bit for bit."""
    on = run_child(spec, {})
    off = run_child(spec, {"MOGP_REPLICA_CACHE": "0"})
    assert on["last_fit"]["replica_engines_reused"] == 1 and on["process"]["replica_engines_reused"] == 1, on
    assert off["process"]["replica_engines_reused"] == 0, off
    assert on["last_fit"]["retargets"] > 0 and off["last_fit"]["retargets"] > 0
    check_oracle(spec, on)
    for k in range(len(on["theta"])):
        assert np.array_equal(on["theta"][k], off["theta"][k]), (k, on["theta"][k], off["theta"][k])
        assert on["logpost"][k] == off["logpost"][k], (k, on["logpost"][k], off["logpost"][k])
    if restored:
        # the slots the pivoted fit left in pivot order went back to training order when the engine was taken again
        assert (on["last_fit"]["replica_inputs_restored"] or 0) > 0, on


# ---------------------------------------------------------------------------------------------------------------------------------
# A. the cached engine taken with other inputs and an analytic mean: H(X) has to be rebuilt
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nugget", [(200, "fit"), (200, 1e-4), (126, "fit")])
def test_reuse_with_other_inputs_rebuilds_the_analytic_mean_design_matrix(n, nugget):
    # n = 126 with three mean terms: n + R = 130 crosses the 128 tile (NP = 256)
    terms = [[0, 1], [1, 1]]
    fits = [dict(seed=100 + n, nugget=nugget, terms=terms, n_tries=4), dict(seed=200 + n, nugget=nugget, terms=terms, n_tries=4)]
    check_reuse(spec_of(fits, n=n))


# ---------------------------------------------------------------------------------------------------------------------------------
# B. a fit of another nugget type after a pivoted fit of the same shape: the slots' inputs must be back in training order
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same_inputs", [True, False], ids=["same_X", "other_X"])
@pytest.mark.parametrize("nugget", ["fit", 1e-6, "adaptive"])
def test_non_pivot_fit_after_a_pivot_fit_of_the_same_shape(nugget, same_inputs):
    fits = [dict(seed=300, nugget="pivot", n_tries=8), dict(seed=300 if same_inputs else 301, nugget=nugget, n_tries=8)]
    check_reuse(spec_of(fits), restored=True)


def test_pivot_fit_after_a_pivot_fit_with_other_inputs():
    # guard: the pivoted factorisation permutes the (refreshed) training-order inputs itself
    fits = [dict(seed=300, nugget="pivot", n_tries=8), dict(seed=302, nugget="pivot", n_tries=8)]
    check_reuse(spec_of(fits))


def test_emulator_switched_from_pivot_to_fixed_nugget_vs_oracle():
    # the same engine, no replica: one emulator fit with pivoting, then with a fixed nugget
    import mogp_emulator_amd as M
    X, T = make_data(303, 150, 3, 1)
    theta = np.array([2.0, 1.5, 0.5, 0.2])
    gp = M.GaussianProcessGPU(X, T[0], nugget="pivot", priors=priors(3, "pivot"))
    gp.fit(theta)
    assert sorted(gp.P) == list(range(150)) and list(gp.P) != list(range(150))
    gp.nugget = 1e-6
    gp.fit(theta)
    rpri = R.GPPriorsRef(3, "fixed", corr=[R.Prior("invgamma", *CORR_PRIOR)] * 3, cov=R.Prior("invgamma", *COV_PRIOR))
    ref = R.GPRef(X, T[0], nugget=1e-6, priors=rpri)
    assert_allclose(gp.current_logpost, ref.fit(theta), rtol=1e-8)
    assert_allclose(gp.logpost_deriv(theta), ref.logpost_deriv(theta), rtol=1e-6, atol=1e-6)
    assert list(gp.P) == list(range(150))
    Xs = make_data(304, 50, 3, 1)[0]
    mean, var, _ = gp.predict(Xs, deriv=False)
    mu, v, _ = ref.predict(Xs)
    assert_allclose(mean, mu, rtol=1e-7, atol=1e-9)
    assert_allclose(var, v, rtol=1e-6, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. pivoted, fixed and fitted nuggets in one replica pool: slots go from pivot runs to others and back
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mixed_nugget_types_share_the_replica_slots():
    # six outputs, 5 starts each, 8 slots: 30 runs, every slot is handed from emulator to emulator.  Emulators 1 and 4 pivot; the
    # design repeats 4 points, so their rank is below n and the rows of L^-1 of the skipped pivots (w2) take part in the gradient.
    # Within one fit a non-pivot run in a slot left in pivot order only wastes its start (it optimises scrambled data and loses to
    # the emulator's start 0, which always runs on an untouched slot), so an all-pivot fit of the same shape goes first: the mixed
    # fit takes its engine with every slot in pivot order, and retargets between pivot and non-pivot runs follow on top.
    first = dict(seed=399, nugget="pivot", n_tries=5, multi=True, repeats=4)
    fit = dict(seed=400, nugget="fit", n_tries=5, multi=True, repeats=4, switch={"1": "pivot", "4": "pivot", "2": 1e-6})
    spec = spec_of([first, fit], n=160, D=3, n_out=6, kernel="Matern52")
    pool = run_child(spec, {"MOGP_START_REPLICAS": "8"})
    own = run_child(spec, {"MOGP_PARALLEL_STARTS": "0"})
    assert pool["last_fit"]["replica_engines_reused"] == 1 and own["process"]["replica_engines_reused"] == 0
    assert pool["last_fit"]["retargets"] > 8, pool
    assert own["last_fit"]["retargets"] == 0, own
    assert pool["nugget"] == ["fit", "pivot", "fixed", "fit", "pivot", "fit"]
    assert pool["rank"][1] < 160 and pool["rank"][4] < 160, pool["rank"]
    check_oracle(spec, pool)
    assert_allclose(pool["logpost"], own["logpost"], rtol=1e-9)
    # (the end points agree to the optimiser's tolerance; a run on inputs in another order ends 0.1 - 1 away)
    for k in range(6):
        assert_allclose(pool["theta"][k], own["theta"][k], rtol=1e-6, atol=1e-9, err_msg="emulator %d" % k)
    # the 8 slots of the all-pivot fit went back to training order when the engine was taken again (at most 8), and slots that ran a
    # pivoted emulator of the mixed fit went back for the next one (the rest)
    assert (pool["last_fit"]["replica_inputs_restored"] or 0) > 8, pool


# ---------------------------------------------------------------------------------------------------------------------------------
# D. both at once: analytic mean and pivoting, then the same mean with a fitted nugget on other inputs through the cache
# ---------------------------------------------------------------------------------------------------------------------------------
def test_analytic_mean_fit_after_pivot_fit_with_other_inputs():
    terms = [[0, 1], [1, 1]]
    fits = [dict(seed=500, nugget="pivot", terms=terms, n_tries=8), dict(seed=501, nugget="fit", terms=terms, n_tries=8)]
    check_reuse(spec_of(fits), restored=True)
