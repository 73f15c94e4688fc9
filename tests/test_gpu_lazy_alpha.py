"""alpha = K^-1 t as cached state of the engine (GPState::alpha, Engine::ensure_alpha): an objective-only evaluation factorises and
forms log det K and |L^-1 t|^2 but leaves the back substitution to whoever reads alpha first.  The shapes are chosen for the places the
deferred one-launch chain can go wrong (d = 3, fixed nugget 1e-6):
    B   n
    1  127   NP = 128: one tile, one chain chunk, the target row is the tile's last row
    3  128   NP = 256: the target row opens a new tile
    9  300   three block columns, chain-bound launch
   70  300   two workgroups per CU, logdet_kernel behind the chain
Everything lazy is compared BIT FOR BIT with the eager path (eval(grad=True) solves alpha with the evaluation): the chain kernel, its
inputs and the sums' device function are the same, so anything but equality is a bug."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, _capi
from mogp_emulator_amd.Priors import GPPriors

pytestmark = pytest.mark.gpu

D, NUG, MQ = 3, 1e-6, 37
SHAPES = [(1, 127), (3, 128), (9, 300), (70, 300)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counter(name):
    c = ctypes.c_longlong()
    assert _capi.load().mogp_profile_counter(name.encode(), ctypes.byref(c)) == 0
    return c.value


def synth(seed, n, d, n_out, m):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, d))
    T = np.empty((n_out, n))
    for k in range(n_out):
        w = rng.normal(size=d)
        T[k] = np.sin(2 * np.pi * X @ w / np.sqrt(d)) + 0.1 * (X ** 2) @ np.abs(w) + 0.01 * rng.normal(size=n)
    return X, T, rng.uniform(0, 1, (m, d))


def problem(B, n):
    X, T, Xs = synth(1000 * B + n, n, D, B, MQ)
    # length scales exp(-raw / 2) = 0.17, 0.14, 0.22: cond(K + 1e-6 I) is 1e4 at n = 127 / 128 and 6e6 at n = 300 (numpy, on the host), so
    # the oracle's means are good to ~1e-9 relative and the suite's bar for means (rtol 1e-7) has room
    theta = np.tile(np.array([3.5, 4.0, 3.0, 0.3]), (B, 1)) + 0.01 * np.arange(B)[:, None]
    return X, T, Xs, theta


def model(X, T, **kw):
    kw.setdefault("nugget", NUG)
    return M.MultiOutputGP_GPU(X, T, priors=GPPriors(n_corr=D, nugget_type="fixed" if kw["nugget"] == NUG else kw["nugget"]), **kw)


def invQt(mo, k):
    out = np.zeros(mo.n)
    mo._mogp_gpu.emulator(k).get_invQt(out)
    return out


@pytest.mark.parametrize("B,n", SHAPES)
def test_objective_only_evaluations_do_not_solve_alpha_and_readers_do_once(B, n):
    X, T, Xs, theta = problem(B, n)
    mo = model(X, T)
    g = mo._mogp_gpu
    c = counter("alpha_solves")
    f0, _, ok = g.eval(theta, grad=False)
    assert ok.all()
    assert counter("alpha_solves") - c == 0
    m1, v1, _ = mo.predict(Xs, deriv=False)
    assert counter("alpha_solves") - c == B
    m2, v2, _ = mo.predict(Xs, deriv=False)
    assert counter("alpha_solves") - c == B
    assert np.all(np.isfinite(m1)) and np.array_equal(m1, m2) and np.array_equal(v1, v2)
    f1, g1, ok = g.eval(theta, grad=True)
    assert ok.all() and np.all(np.isfinite(g1))
    assert counter("alpha_solves") - c == 2 * B
    assert np.array_equal(f0, f1)
    # a subset evaluated without gradient: predicting with all of them solves the subset alone
    sub = sorted({0, B // 2, B - 1})
    for k in sub:
        mo.fit_emulator(k, theta[k] + 0.05)
    assert counter("alpha_solves") - c == 2 * B
    m3, _, _ = mo.predict(Xs, deriv=False)
    assert counter("alpha_solves") - c == 2 * B + len(sub)
    rest = [k for k in range(B) if k not in sub]
    assert np.array_equal(m3[rest], m1[rest]) and np.all(np.isfinite(m3))
    for k in sub:
        assert not np.array_equal(m3[k], m1[k])


@pytest.mark.parametrize("B,n", SHAPES)
def test_lazy_alpha_and_predictions_are_the_eager_bits(B, n):
    X, T, Xs, theta = problem(B, n)
    lazy, eager = model(X, T), model(X, T)
    f0, _, ok0 = lazy._mogp_gpu.eval(theta, grad=False)
    lazy.fit(theta)
    f1, _, ok1 = eager._mogp_gpu.eval(theta, grad=True)
    assert ok0.all() and ok1.all()
    assert np.array_equal(f0, f1)
    ml, vl, _ = lazy.predict(Xs, deriv=False)
    me, ve, _ = eager.predict(Xs, deriv=False)
    assert np.all(np.isfinite(ml)) and np.all(np.isfinite(vl))
    assert np.array_equal(ml, me) and np.array_equal(vl, ve)
    for k in range(B):
        a = invQt(lazy, k)
        assert np.all(np.isfinite(a))
        assert np.array_equal(a, invQt(eager, k))


def _after(B, n, how):
    """a fresh model at theta: how = "fit" (alpha deferred) or "grad" (alpha solved with the evaluation)"""
    X, T, Xs, theta = problem(B, n)
    mo = model(X, T)
    if how == "fit":
        mo.fit(theta)
    else:
        _, _, ok = mo._mogp_gpu.eval(theta, grad=True)
        assert ok.all()
    return mo, Xs, theta


def _deriv(mo, Xs, theta):
    return mo.predict(Xs, unc=False, deriv=True).deriv


def _gradient(mo, Xs, theta):
    out = np.zeros((mo.n_emulators, theta.shape[1]))
    for k in range(mo.n_emulators):
        mo._mogp_gpu.emulator(k).logpost_deriv(out[k])
    return out


def _hessian(mo, Xs, theta):
    H, ok = mo._mogp_gpu.hessian(theta)
    assert ok.all()
    return H


def _loo(mo, Xs, theta):
    return np.concatenate([np.ravel(a) for a in mo._mogp_gpu.cross_validate(np.arange(mo.n), mo.n)])


def _kfold(mo, Xs, theta):
    return np.concatenate([np.ravel(a) for a in mo._mogp_gpu.cross_validate(np.arange(mo.n) % 3, 3)])


def _full_cov(mo, Xs, theta):
    r = mo.predict(Xs, deriv=False, full_cov=True)
    return np.concatenate([np.ravel(r.mean), np.ravel(r.unc)])


def _implausibility(mo, Xs, theta):
    B = mo.n_emulators
    return mo._mogp_gpu.implausibility(Xs, 0.1 * np.arange(B), 0.01, 0.02, True, min(1, B - 1))


READERS = {"predict_deriv": _deriv, "logpost_deriv": _gradient, "logpost_hessian": _hessian, "cross_validate_loo": _loo,
           "cross_validate_3fold": _kfold, "predict_full_cov": _full_cov, "implausibility": _implausibility}


@pytest.mark.parametrize("reader", list(READERS))
@pytest.mark.parametrize("B,n", SHAPES)
def test_every_reader_of_alpha_gives_the_eager_numbers_right_after_a_plain_fit(B, n, reader):
    fn = READERS[reader]
    lazy, Xs, theta = _after(B, n, "fit")
    c = counter("alpha_solves")
    got = np.asarray(fn(lazy, Xs, theta), dtype=np.float64)
    assert counter("alpha_solves") - c == B, "the reader did not ask for alpha"
    eager, _, _ = _after(B, n, "grad")
    want = np.asarray(fn(eager, Xs, theta), dtype=np.float64)
    assert np.all(np.isfinite(got)), "a reader saw the sentinel rows"
    assert np.array_equal(got, want), np.nanmax(np.abs(got - want))


_LINESEARCH_SCRIPT = r"""
import sys, ctypes, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import mogp_emulator_amd as M
from mogp_emulator_amd import libgpgpu, _capi
from test_gpu_lazy_alpha import synth, counter
X, T, _ = synth(4243, 300, 3, 9, 8)
libgpgpu.set_fit_options(max_iter=40, ftol=1e-9, gtol=1e-6, seed=11)
mo = M.fit_GP_MAP(M.MultiOutputGP_GPU(X, T, nugget=1e-6), n_tries=3)
assert mo.get_indices_not_fit() == []
m = mo.predict(X[:5] + 0.01, unc=False, deriv=False).mean
assert np.all(np.isfinite(m))
print("COUNTS", counter("alpha_solves"), counter("objective_evals"), counter("gradient_evals"), counter("backsolve_timeouts"))
print("OPTIMA", " ".join(repr(float(em.current_logpost)) for em in mo.emulators))
"""


_line_search_runs = {}


def _line_search(**env):
    """(counters [alpha_solves, objective_evals, gradient_evals, backsolve_timeouts], optima) of _LINESEARCH_SCRIPT in a child process with
    `env`; every setting runs once per session"""
    key = tuple(sorted(env.items()))
    if key not in _line_search_runs:
        script = _LINESEARCH_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
        out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "OPTIMA" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
        counts = [int(x) for x in out.stdout.split("COUNTS")[1].split()[:4]]
        print("%s alpha_solves, objective_evals, gradient_evals, backsolve_timeouts = %s" % (env, counts))
        _line_search_runs[key] = (counts, np.array([float(x) for x in out.stdout.split("OPTIMA")[1].split()]))
    return _line_search_runs[key]


def test_lazy_gradient_line_search_solves_alpha_only_where_it_takes_a_gradient():
    """fit_GP_MAP with the objective-first line search (MOGP_LAZY_GRAD=1: the default from n = 512, forced here at n = 300) and with
    objective and gradient in one evaluation (=0), each in a child process: the same optima to the tolerance test_gpu_parity.py holds
    that switch to (rtol 1e-6 on the log-posterior), and with =1 fewer alpha solves than objective evaluations -- the trial points that
    fail the sufficient-decrease test and the final refit take none."""
    lazy, eager = _line_search(MOGP_LAZY_GRAD="1"), _line_search(MOGP_LAZY_GRAD="0")
    assert_allclose(lazy[1], eager[1], rtol=1e-6)
    alpha_solves, objective_evals, gradient_evals, timeouts = lazy[0]
    assert alpha_solves < objective_evals
    # one solve per gradient, plus the 9 emulators of the final prediction
    assert alpha_solves == gradient_evals + 9
    assert timeouts == 0 and eager[0][3] == 0


def test_line_search_gradients_behind_timed_out_chains_are_solved_again():
    """The gradient route of a time-out, batched as the line search runs it: with MOGP_BS_SPIN=0 the chains grad_current issues under the
    triangular inversion (up to 27 emulators x 3 chunks per launch, a launch per optimiser round) give up wherever a value is not there
    at the first poll.  The time-out words come back with the gradient; grad_current must repeat those solves with the multi-launch path,
    count them, and compute the gradient again -- the fit then ends where the fit without forced time-outs ends (rtol 1e-6 on the
    log-posterior: the tolerance test_gpu_parity.py holds alpha-by-another-path to).  A gradient taken from a timed-out alpha would send
    the search elsewhere."""
    forced, plain = _line_search(MOGP_LAZY_GRAD="1", MOGP_BS_SPIN="0"), _line_search(MOGP_LAZY_GRAD="1")
    assert forced[0][3] > 0, "the forced time-outs never happened: the repeat under the gradient was not exercised"
    assert_allclose(forced[1], plain[1], rtol=1e-6)


@pytest.mark.parametrize("B,n", SHAPES)
@pytest.mark.parametrize("what", ["analytic_mean", "pivot"])
def test_analytic_mean_and_pivot_stay_eager(B, n, what):
    X, T, Xs, theta = problem(B, n)
    if what == "analytic_mean":
        mo = model(X, T, mean=LibGPGPU.PolyMeanFunc([(0, 1)]), analytic_mean=True)
    else:
        mo = model(X, T, nugget="pivot")
    c = counter("alpha_solves")
    f, _, ok = mo._mogp_gpu.eval(theta, grad=False)
    assert ok.all()
    assert counter("alpha_solves") - c == B
    m, _, _ = mo.predict(Xs, deriv=False)
    assert counter("alpha_solves") - c == B and np.all(np.isfinite(m))


_TIMEOUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
from oracle import cpu_ref as R
from test_gpu_lazy_alpha import problem, model, counter
# (3, 128): n = 128 is ONE chain chunk, which waits for nobody -- the control: no time-out can happen on either route.
# (9, 300): three chunks per emulator, 18 waits per launch, none of them satisfied at its first poll unless its producer has already finished
for B, n in ((3, 128), (9, 300)):
    waits = (n + 127) // 128 > 1
    X, T, Xs, theta = problem(B, n)
    mo = model(X, T)
    t0, a0 = counter("backsolve_timeouts"), counter("alpha_solves")
    mo.fit(theta)
    assert counter("backsolve_timeouts") == t0 and counter("alpha_solves") == a0      # nothing solved, nothing to time out
    mean, unc, _ = mo.predict(Xs, deriv=False)
    assert counter("alpha_solves") - a0 == B
    d_predict = counter("backsolve_timeouts") - t0
    print("BS-TIMEOUTS-PREDICT", B, n, d_predict)
    assert (d_predict > 0) if waits else (d_predict == 0), "fit -> predict: %%d time-outs at B=%%d n=%%d" %% (d_predict, B, n)
    for k in (0, B - 1):
        ref = R.GPRef(X, T[k], nugget=1e-6)
        ref.fit(theta[k])
        mu, var, _ = ref.predict(Xs)
        print("MEAN-ERR", k, float(np.abs(mean[k] - mu).max()), float(np.abs(mu).max()))
        np.testing.assert_allclose(mean[k], mu, rtol=1e-7, atol=1e-9)
    # the same behind a gradient: the chain runs under the triangular inversion and its time-out words come back with the gradient
    # (the bar test_gpu_parity.py holds gradients against the oracle to: rtol 1e-6, atol 1e-7)
    mo = model(X, T)
    mo.fit(theta)
    t1 = counter("backsolve_timeouts")
    grads = np.zeros(theta.shape)
    for k in range(B):
        mo._mogp_gpu.emulator(k).logpost_deriv(grads[k])
    d_grad = counter("backsolve_timeouts") - t1
    print("BS-TIMEOUTS-GRADIENT", B, n, d_grad)
    # (one emulator per launch here: three workgroups that start together, so whether a wait finds its value at the first poll is a
    # race -- the count is shown, not required; the batched gradient route, where it is required, is the line-search test's)
    assert d_grad >= 0 if waits else d_grad == 0, "fit -> logpost_deriv: %%d time-outs at B=%%d n=%%d" %% (d_grad, B, n)
    for k in (0, B - 1):
        ref = R.GPRef(X, T[k], nugget=1e-6)
        ref.fit(theta[k])
        np.testing.assert_allclose(grads[k], ref.logpost_deriv(theta[k]), rtol=1e-6, atol=1e-7)
print("TIMEOUT-CASES-OK")
"""


def test_a_deferred_chain_that_times_out_is_solved_again():
    """MOGP_BS_SPIN=0 (its own process: the variable is read once) turns every wait of the one-launch chain that is not satisfied at the first
    poll into a time-out.  After a plain fit the chain runs inside the first reader.  fit -> predict (ensure_alpha): `backsolve_timeouts`
    must rise where the chain has more than one chunk (9 x 300: 18 waits in the launch) and stay where it has one (3 x 128, the control),
    and the means must be the oracle's (the suite's bar: rtol 1e-7, atol 1e-9) -- the repeat with the multi-launch path was taken, counted
    and right.  fit -> logpost_deriv of one emulator at a time (grad_current): the gradients must be the oracle's (rtol 1e-6, atol 1e-7)
    whether or not that emulator's chain timed out; the control stays at 0."""
    script = _TIMEOUT_SCRIPT % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MOGP_BS_SPIN="0"), capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "TIMEOUT-CASES-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
