"""Host-side checks of sample_posterior: the NumPy restatement of the normal generator (sample_restate.py) against Random123's known answers
and against the host build of csrc/philox_dev.h; the statistics of the restatement (the device is held to it, so its statistics follow);
sample_plan and the jitter ladder (csrc/predict_plan.h) through a sanitised host program; the argument refusals that need no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU, Sampling

import sample_restate as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 2024


def _build_and_run(tmp_path, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_restatement_reproduces_the_known_answers_and_the_stated_values():
    for ctr, key, want in sr.KAT:
        assert sr.philox_scalar(ctr, key) == want
        got = sr.philox_block(*[np.array([c]) for c in ctr], key[0], key[1])
        assert tuple(int(g[0]) for g in got) == want
        assert tuple(int(x) for x in Sampling.philox4x32_10(np.array(ctr), np.array(key))) == want
    z = sr.normals(SEED, 0, 2, 3)
    np.testing.assert_allclose(z, [[0.99998332, -0.09707058, 1.16680507], [-1.56102521, -0.27281988, -1.21764277]], rtol=0, atol=5e-9)
    # the package's own helper is the same rule
    for stream, S, m in [(0, 3, 1), (2, 7, 129), (5, 4, 128), (2 ** 32 - 1, 2, 5)]:
        assert np.array_equal(Sampling.philox_normals(SEED, stream, S, m), sr.normals(SEED, stream, S, m))
    assert np.array_equal(Sampling.philox_normals(SEED, 1, 3, 9, first_draw=4), sr.normals(SEED, 1, 7, 9)[4:])


def test_host_build_of_the_generator_matches_the_restatement(tmp_path):
    """The words exactly; the normals to 1e-13 absolute: two libms may differ by a few ulp in log and cos, at |z| <= 8.6."""
    out = _build_and_run(tmp_path, "philox_check")
    kat = [tuple(int(w, 16) for w in ln.split()[1:]) for ln in out.splitlines() if ln.startswith("kat")]
    assert kat == [want for _, _, want in sr.KAT]
    rows = [ln.split() for ln in out.splitlines() if ln.startswith("z ")]
    assert [int(r[1]) for r in rows] == list(range(7))
    z = np.array([[float(v) for v in r[2:]] for r in rows])
    assert z.shape == (7, 129)
    ref = sr.normals(SEED, 2, 7, 129)
    dis = np.max(np.abs(z - ref))
    print("host build against the NumPy restatement: %.3g (bar 1e-13)" % dis)
    assert dis <= 1e-13


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_statistics_of_the_restatement(stream):
    S, m = 4096, 8
    Z = sr.normals(SEED, stream, S, m)
    G = Z.T @ Z / S - np.eye(m)
    se = np.sqrt((1. + np.eye(m)) / S)
    print("stream %d: largest |Z^T Z / S - I| in standard errors %.2f" % (stream, np.max(np.abs(G) / se)))
    assert np.all(np.abs(G) <= 4. * se)
    N = 1024
    B = sr.normals(SEED, stream, N, N).ravel()
    n = B.size
    # standard errors of the sample mean, second and fourth moment of a standard normal: 1, sqrt(2), sqrt(96) over sqrt(n)
    dev = [abs(B.mean()) / np.sqrt(1. / n), abs(np.mean(B ** 2) - 1.) / np.sqrt(2. / n), abs(np.mean(B ** 4) - 3.) / np.sqrt(96. / n)]
    print("stream %d: mean, variance, fourth moment off by %.2f, %.2f, %.2f standard errors" % (stream, *dev))
    assert max(dev) <= 4.
    assert np.all(np.isfinite(B)) and np.max(np.abs(B)) <= 8.6


def test_a_value_depends_on_seed_stream_draw_and_point_alone():
    a = sr.normals(SEED, 2, 7, 129)
    assert np.array_equal(a[:, :128], sr.normals(SEED, 2, 7, 128))
    assert np.array_equal(a[:3], sr.normals(SEED, 2, 3, 129))
    assert np.array_equal(a[:, :127], sr.normals(SEED, 2, 7, 127))          # an odd m drops the last sine, nothing else
    assert not np.array_equal(a, sr.normals(SEED, 3, 7, 129))
    assert not np.array_equal(a, sr.normals(SEED + 1, 2, 7, 129))
    assert not np.array_equal(a, sr.normals(SEED + 2 ** 32, 2, 7, 129))     # the high word of the seed is in the key


def test_restated_ladder():
    rng = np.random.default_rng(3)
    m = 40
    A = rng.normal(size=(m, m))
    cov = A @ A.T / m + 0.1 * np.eye(m)
    mu, z = rng.normal(size=m), rng.normal(size=(5, m))
    y, ju, ok, St = sr.sample(mu, cov, z, nugget=1e-3, jitter=1e-4)
    assert ok and ju == 1e-4 and np.allclose(St, cov + (1e-3 + 1e-4) * np.eye(m))
    L = np.linalg.cholesky(St)
    np.testing.assert_allclose(y, mu + z @ L.T, rtol=0, atol=1e-13)
    # rank one and no nugget: the first try may or may not fail in floating point; the invariants hold either way
    one = np.full((m, m), 0.7)
    y, ju, ok, St = sr.sample(mu, one, z)
    assert ok and np.all(np.isfinite(y))
    assert ju == 0. or any(np.isclose(ju, sr.ladder_delta(t, 0.7), rtol=1e-12, atol=0) for t in range(5))
    # not positive definite beyond the last rung
    bad = -np.eye(m)
    y, ju, ok, St = sr.sample(mu, bad, z)
    assert not ok and np.all(np.isnan(y))
    for t in range(5):
        assert np.isclose(sr.ladder_delta(t, 2.5), 1e-6 * 10. ** t * 2.5, rtol=1e-14, atol=0)


def test_sample_plan_properties(tmp_path):
    """tests/c/sample_plan_check.cpp sweeps (E, m, S, n, free bytes, max_slots, max_draws) itself and exits non-zero at the first property
    that fails; built with the address and undefined-behaviour sanitisers"""
    assert "cases ok" in _build_and_run(tmp_path, "sample_plan_check")


class _Native(object):
    "what sample_posterior reads of the native object before it calls into the library"
    def __init__(self, D, fitted=True):
        self._D, self._fitted = D, fitted

    def D(self):
        return self._D

    def theta_fit_status(self):
        return self._fitted

    def sample_posterior(self, *a, **kw):
        raise AssertionError("the device must not be reached")


def _stub(D=3, nugget=2, fitted=True, analytic=False):
    gp = M.GaussianProcessGPU.__new__(M.GaussianProcessGPU)
    gp._densegp_gpu = _Native(D, fitted)
    gp._nugget_type = LibGPGPU.nugget_type(nugget)
    gp._analytic_mean = analytic
    return gp


def test_sample_posterior_refusals_without_a_device():
    with pytest.raises(TypeError):
        M.sample_posterior(object(), np.zeros((2, 3)))
    gp = _stub()
    X = np.linspace(0., 1., 12).reshape(4, 3)
    nanX, infZ = X.copy(), np.zeros((2, 4))
    nanX[1, 2] = np.nan
    infZ[0, 0] = np.inf
    for args, kw in [((np.zeros((4, 2)),), {}), ((np.zeros((0, 3)),), {}), ((np.zeros((2, 2, 3)),), {}), ((nanX,), {}), ((X,), dict(n_draws=0)),
                     ((X,), dict(n_draws=-3)), ((X,), dict(jitter=-1e-9)), ((X,), dict(jitter=np.nan)), ((X,), dict(max_slots=-1)),
                     ((X,), dict(max_draws=-1)), ((X,), dict(stream=-1)), ((X,), dict(stream=2 ** 32)), ((X,), dict(z=np.zeros((2, 5)))),
                     ((X,), dict(z=np.zeros(4))), ((X,), dict(z=np.zeros((1, 2, 4)))), ((X,), dict(z=np.zeros((0, 4)))), ((X,), dict(z=infZ))]:
        with pytest.raises(ValueError):
            M.sample_posterior(gp, *args, **kw)
    with pytest.raises(RuntimeError, match="pivot"):
        M.sample_posterior(_stub(nugget=3), X)
    with pytest.raises(RuntimeError, match="analytic_mean"):
        M.sample_posterior(_stub(analytic=True), X)
    with pytest.raises(RuntimeError, match="not been fit"):
        M.sample_posterior(_stub(fitted=False), X)
    # what is valid gets as far as the library
    for kw in [dict(), dict(n_draws=5, rng=1), dict(z=np.zeros((2, 4))), dict(jitter=1e-8, include_nugget=False, stream=7, return_z=True),
               dict(max_slots=2, max_draws=3)]:
        with pytest.raises(AssertionError, match="must not be reached"):
            M.sample_posterior(gp, X, **kw)
    assert Sampling.sample_posterior is M.sample_posterior and M.PosteriorSamples is Sampling.PosteriorSamples


def test_the_seed_is_one_draw_of_the_generator_passed():
    seen = {}

    class Native(_Native):
        def sample_posterior(self, testing, **kw):
            seen.update(kw)
            S, m = kw["n_draws"], testing.shape[0]
            return np.zeros((S, m)), np.zeros(m), None, 0., True

    gp = _stub()
    gp._densegp_gpu = Native(3)
    X = np.zeros((4, 3))
    r = M.sample_posterior(gp, X, n_draws=2, rng=11)
    want = int(np.random.default_rng(11).integers(0, 2 ** 64, dtype=np.uint64))
    assert r.seed == want == seen["seed"] and r.n_draws == 2 and r.z is None
    g = np.random.default_rng(11)
    assert M.sample_posterior(gp, X, rng=g).seed == want
    assert M.sample_posterior(gp, X, rng=g).seed != want                      # the caller's generator advances
    r = M.sample_posterior(gp, X, z=np.zeros((3, 4)), n_draws=99)
    assert r.seed is None and seen["n_draws"] == 3                            # n_draws comes from z
