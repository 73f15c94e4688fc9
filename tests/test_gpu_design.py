"""Designs on the MI355X: the batched minimum pairwise distance against scipy's pdist under a derived bound, seeded MaxiMinLHC samples
equal to the reference's, MICEDesign's candidate scores against the reference's _MICE_criterion at a fixed theta, and the sequential
loop end to end."""
import importlib

import numpy as np
import pytest
from numpy.testing import assert_allclose
from scipy.spatial.distance import pdist

import mogp_emulator_amd as M
from mogp_emulator_amd.ExperimentalDesign import LatinHypercubeDesign, MaxiMinLHC

from design_cases import DESIGN_ARGS, MICE_CASES, N_PARAMETERS, maximin_cases

# the module: the package attribute of this name is the class, as in the reference package
SD = importlib.import_module("mogp_emulator_amd.SequentialDesign") if M.HAVE_LIBGPGPU else None

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def min_pdist_rtol(D):
    """Either side forms a squared distance from D differences (one rounding each), their squares (the difference's error twice, plus
    one rounding) and D - 1 additions of non-negative terms: relative error below (D + 2) u, u = 2^-53; the square root halves that and
    adds one rounding -- below (D + 2) u again.  The minimum of values that each moved by at most that factor moved by no more.  Two
    sides: 2 (D + 2) u."""
    return 2.0 * (D + 2) * U


def scipy_min(designs):
    return np.array([pdist(d).min() for d in designs])


# ---- design_min_pdist -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 2000])
@pytest.mark.parametrize("D", [1, 10, 80])
@pytest.mark.parametrize("T", [1, 7, 300])
def test_min_pdist_against_scipy(n, D, T):
    from mogp_emulator_amd import libgpgpu
    rng = np.random.default_rng(1000003 * n + 1009 * D + T)
    designs = rng.uniform(0., 1., (T, n, D))
    got = libgpgpu.design_min_pdist(designs)
    want = scipy_min(designs)
    assert got.shape == (T,) and got.dtype == np.float64
    worst = np.max(np.abs(got - want) / want)
    print("n=%d D=%d T=%d: largest relative difference %.3g (bound %.3g)" % (n, D, T, worst, min_pdist_rtol(D)))
    assert_allclose(got, want, rtol=min_pdist_rtol(D), atol=0.)


def test_min_pdist_in_two_chunks():
    """More designs than one pass over the device takes (64 MiB of designs per pass): the result does not show the seam."""
    from mogp_emulator_amd import libgpgpu
    n, D = 129, 80
    per_pass = (64 << 20) // (8 * n * D)
    T = per_pass + 37
    rng = np.random.default_rng(77)
    designs = rng.uniform(-3., 5., (T, n, D))
    got = libgpgpu.design_min_pdist(designs)
    assert_allclose(got, scipy_min(designs), rtol=min_pdist_rtol(D), atol=0.)
    # each design on its own gives the same bits as in the batch (a minimum has no order), on either side of the seam
    for t in (0, per_pass - 1, per_pass, T - 1):
        assert libgpgpu.design_min_pdist(designs[t])[0] == got[t]


def test_min_pdist_repeated_point_is_exactly_zero():
    from mogp_emulator_amd import libgpgpu
    rng = np.random.default_rng(5)
    for n, D, i, j in ((2, 3, 0, 1), (65, 10, 64, 3), (200, 80, 130, 129), (2000, 10, 1999, 7)):
        designs = rng.uniform(0., 1., (3, n, D))
        designs[1, i] = designs[1, j]
        got = libgpgpu.design_min_pdist(designs)
        assert got[1] == 0.0 and got[0] > 0. and got[2] > 0.


def test_min_pdist_accepts_one_design_and_rejects_bad_shapes():
    from mogp_emulator_amd import libgpgpu
    X = np.array([[0., 0.], [3., 4.], [10., 10.]])
    assert libgpgpu.design_min_pdist(X).tolist() == [5.0]
    assert libgpgpu.design_min_pdist(X[None, :, :1].repeat(2, axis=0)).tolist() == [3.0, 3.0]
    with pytest.raises(ValueError):
        libgpgpu.design_min_pdist(X[:1])
    with pytest.raises(RuntimeError, match="dimensions"):
        libgpgpu.design_min_pdist(np.zeros((1, 4, 81)))


# ---- MaxiMinLHC ---------------------------------------------------------------------------------------------------------------------------
def test_maximin_equals_the_reference(golden):
    from mogp_emulator_amd import libgpgpu
    g = golden("design.npz")
    cases = maximin_cases(g)
    assert len(cases) == 6
    for key, name, n, n_tries, seed in cases:
        np.random.seed(seed)
        got = MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries)
        assert np.array_equal(got, g[key]), key
        # every try's distance against the one scipy computed for the reference
        D = N_PARAMETERS[name]
        np.random.seed(seed)
        tries = np.array([LatinHypercubeDesign(D)._draw_samples(n) for _ in range(n_tries)])
        assert_allclose(libgpgpu.design_min_pdist(tries), g[key + "_mins"], rtol=min_pdist_rtol(D), atol=0.)


def test_maximin_in_chunks_equals_the_reference(golden, monkeypatch):
    g = golden("design.npz")
    key, name, n, n_tries, seed = [c for c in maximin_cases(g) if c[3] == 1000][0]
    monkeypatch.setattr(MaxiMinLHC, "CHUNK_BYTES", 300 * 8 * n * N_PARAMETERS[name])
    np.random.seed(seed)
    assert np.array_equal(MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries), g[key])


# ---- MICEDesign -----------------------------------------------------------------------------------------------------------------------------
def _mice_at_golden(g, name, monkeypatch):
    inputs, targets, cand = g["mice_%s_inputs" % name], g["mice_%s_targets" % name], g["mice_%s_candidates" % name]
    theta = g["mice_%s_theta" % name]
    md = SD.MICEDesign(LatinHypercubeDesign(inputs.shape[1]), n_init=len(inputs), n_cand=len(cand),
                       nugget=float(g["mice_%s_nugget" % name]), nugget_s=float(g["mice_%s_nugget_s" % name]))
    md.inputs, md.targets, md.candidates = inputs, targets, cand
    md.current_iteration, md.initialized = len(inputs), True
    fits = []

    def fixed_fit(gp, **kw):          # optimiser end points are not pinned: the golden values are at this theta
        fits.append(gp)
        gp.fit(theta)
        return gp
    monkeypatch.setattr(SD, "fit_GP_MAP", fixed_fit)
    return md, fits


@pytest.mark.parametrize("name", MICE_CASES)
def test_mice_scores_against_the_reference(golden, monkeypatch, name):
    """rtol = 1e-6, as tests/test_gpu_parity.py::test_mice_criterion_vs_reference uses for the same quantity.  The reference subtracts two
    nearly equal numbers for the denominator, so the committed cases are ones where the reference itself is within 2.5e-7 of a
    long-double evaluation (asserted by tests/golden/make_golden_design.py; at nugget 1e-4 with 400 candidates it is 2.8e-6 away, and
    the device then differs from it by exactly that much)."""
    g = golden("design.npz")
    md, fits = _mice_at_golden(g, name, monkeypatch)
    want = g["mice_%s_crit" % name]
    calls = []
    real = SD.mice_criterion
    monkeypatch.setattr(SD, "mice_criterion", lambda *a, **k: calls.append(1) or real(*a, **k))
    best = md._eval_metric()
    assert len(fits) == 1 and isinstance(md.gp, M.GaussianProcessGPU) and len(calls) == 1       # one fit, ONE scoring call
    print("%s: largest relative difference %.3g" % (name, np.max(np.abs(md._scores - want) / want)))
    assert_allclose(md._scores, want, rtol=1e-6)
    assert best == int(np.argmax(want))
    # the reference's per-point call reads the kept vector
    for i in (0, len(want) // 2, len(want) - 1):
        assert md._MICE_criterion(i) == md._scores[i]
    assert len(calls) == 1
    md._scores = None
    assert_allclose(md._MICE_criterion(3), want[3], rtol=1e-6)
    assert len(calls) == 2
    assert_allclose(md._estimate_next_target(md.candidates[best]), g["mice_%s_next_target" % name], rtol=1e-7, atol=1e-9)


def test_mice_retries_a_failed_fit(golden, monkeypatch):
    g = golden("design.npz")
    md, fits = _mice_at_golden(g, "c50", monkeypatch)
    theta = g["mice_c50_theta"]
    attempts = []

    def flaky(gp, **kw):
        attempts.append(1)
        if len(attempts) < 3:
            raise RuntimeError("GP fitting failed")
        gp.fit(theta)
        return gp
    monkeypatch.setattr(SD, "fit_GP_MAP", flaky)
    assert md._eval_metric() == int(np.argmax(g["mice_c50_crit"])) and len(attempts) == 3

    def hopeless(gp, **kw):
        attempts.append(1)
        raise RuntimeError("GP fitting failed")
    del attempts[:]
    monkeypatch.setattr(SD, "fit_GP_MAP", hopeless)
    with pytest.raises(RuntimeError, match="Unable to find parameters"):
        md._eval_metric()
    assert len(attempts) == 10


def test_mice_raises_other_errors_unchanged(golden, monkeypatch):
    """Only a failed fit or factorisation is tried again; anything else the library raises reaches the caller at once, as it is."""
    g = golden("design.npz")
    md, fits = _mice_at_golden(g, "c50", monkeypatch)
    attempts = []

    def broken(gp, **kw):
        attempts.append(1)
        raise RuntimeError("HIP error in hipMemcpy: an illegal memory access was encountered")
    monkeypatch.setattr(SD, "fit_GP_MAP", broken)
    with pytest.raises(RuntimeError, match="HIP error in hipMemcpy"):
        md._eval_metric()
    assert len(attempts) == 1
    # a candidate matrix that cannot be factorised IS such a failure: ten attempts, the cause kept
    md2, _ = _mice_at_golden(g, "c50", monkeypatch)
    md2.nugget, md2.nugget_s = 0., 1.
    md2.candidates = np.repeat(md2.candidates[:25], 2, axis=0)          # every candidate twice, no nugget
    with pytest.raises(RuntimeError, match="Unable to find parameters") as err:
        md2._eval_metric()
    assert "factoriz" in str(err.value.__cause__)


def simulator(x):
    return np.sin(3.0 * x[0]) + x[1] * x[1]


def test_run_sequential_design_end_to_end():
    from mogp_emulator_amd import MICEDesign
    np.random.seed(42)
    md = MICEDesign(MaxiMinLHC(2, (0., 2.)), f=simulator, n_samples=4, n_init=8, n_cand=40, nugget=1.e-6)
    seen = []
    draw = md._generate_candidates

    def keep():
        draw()
        seen.append(md.get_candidates().copy())
    md._generate_candidates = keep
    md.run_sequential_design()
    assert md.get_current_iteration() == 12 and len(seen) == 4
    X, y = md.get_inputs(), md.get_targets()
    assert X.shape == (12, 2) and y.shape == (12,) and np.all((X >= 0.) & (X <= 2.))
    for step, cand in enumerate(seen):
        assert cand.shape == (40, 2)
        assert np.any(np.all(cand == X[8 + step], axis=1))           # the chosen point is one of that step's candidates
    assert np.array_equal(y, [simulator(x) for x in X])
    assert md._scores.shape == (40,) and np.all(np.isfinite(md._scores))


def test_batch_points_on_the_device():
    from mogp_emulator_amd import MICEDesign
    np.random.seed(43)
    md = MICEDesign(LatinHypercubeDesign(2), f=simulator, n_init=10, n_cand=500, nugget=1.e-6, nugget_s=2.)
    md.run_initial_design()
    y0 = md.get_targets().copy()
    batch = md.get_batch_points(3)
    assert batch.shape == (3, 2) and len(np.unique(batch, axis=0)) == 3
    assert md.get_inputs().shape == (13, 2) and np.array_equal(md.get_inputs()[10:], batch)
    assert md.get_current_iteration() == 10 and np.array_equal(md.get_targets(), y0)
    # the last emulator of the batch was fitted with the first two stand-in targets in place
    assert md.gp.n == 12 and np.array_equal(md.gp.targets[:10], y0)
    md.set_batch_targets([simulator(x) for x in batch])
    assert md.get_current_iteration() == 13 and md.get_targets().shape == (13,)
    md.run_next_point()
    assert md.get_current_iteration() == 14 and md.get_targets()[-1] == simulator(md.get_inputs()[-1])
