"""Experimental and sequential designs on the host: surface, argument forms and errors of the four one-shot classes, seeded Monte-Carlo
and Latin-hypercube samples EQUAL to the reference's, the maximin selection with the device call replaced by scipy, the loud failure
without a GPU, and the bookkeeping of SequentialDesign with a stub metric."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.ExperimentalDesign import ExperimentalDesign, LatinHypercubeDesign, MaxiMinLHC, MonteCarloDesign

from design_cases import DESIGN_ARGS, N_PARAMETERS, maximin_cases, oneshot_cases, ppf_quadratic

ALL = (ExperimentalDesign, MonteCarloDesign, LatinHypercubeDesign, MaxiMinLHC)


# ---- construction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ALL)
def test_argument_forms(cls):
    for name, args in DESIGN_ARGS.items():
        d = cls(*args)
        assert d.get_n_parameters() == N_PARAMETERS[name] == len(d.distributions)
    d = cls(3)
    assert [f(0.25) for f in d.distributions] == [0.25] * 3
    d = cls(2, (-1.0, 3.0))
    assert [f(0.25) for f in d.distributions] == [0.0, 0.0]
    d = cls(2, [2, 4])                                  # any two-number iterable is a pair of bounds
    assert [f(0.5) for f in d.distributions] == [3.0, 3.0]
    d = cls(2, [(0., 1.), (2., 4.)])                    # ... and a list of pairs one entry per parameter
    assert [f(0.5) for f in d.distributions] == [0.5, 3.0]
    d = cls([ppf_quadratic, (2.0, 2.5)])
    assert d.distributions[0] is ppf_quadratic and d.distributions[1](1.0) == 2.5
    d = cls(np.array([[0., 2.], [1., 2.]]))             # an array of bounds is iterated like a list
    assert [f(0.5) for f in d.distributions] == [1.0, 1.5]


@pytest.mark.parametrize("cls", ALL)
def test_argument_errors(cls):
    with pytest.raises(ValueError):
        cls()
    with pytest.raises(ValueError):
        cls(1, (0., 1.), 3)
    with pytest.raises(TypeError):
        cls(None)
    with pytest.raises(TypeError):
        cls([1, 2], (0., 1.))
    with pytest.raises(TypeError):
        cls(2, 5)
    with pytest.raises(ValueError):
        cls(0)
    with pytest.raises(ValueError):
        cls(-2, (0., 1.))
    with pytest.raises(ValueError):
        cls(2, (1., 1.))
    with pytest.raises(ValueError):
        cls(2, (2., 1.))
    with pytest.raises(ValueError):
        cls(2, lambda a, b: a)
    with pytest.raises(ValueError):
        cls(3, [(0., 1.), (0., 1.)])
    with pytest.raises(ValueError):
        cls([(0., 1.), (3., 2.)])
    with pytest.raises(ValueError):
        cls([(0., 1.), (0., 1., 2.)])
    with pytest.raises(ValueError):
        cls([(0., 1.), lambda a, b: a])
    with pytest.raises(TypeError):
        cls([(0., 1.), 3.])
    with pytest.raises(TypeError):
        cls([(0., 1.), (None, 2.)])


def test_method_and_str():
    base = ExperimentalDesign(3)
    with pytest.raises(NotImplementedError):
        base.get_method()
    with pytest.raises(NotImplementedError):
        base.sample(3)
    assert str(base) == "Experimental Design with 3 parameters"
    # a MaxiMinLHC reports its parent's method, as the reference's does (the parent's constructor sets the attribute last)
    for cls, method in ((MonteCarloDesign, "Monte Carlo"), (LatinHypercubeDesign, "Latin Hypercube"), (MaxiMinLHC, "Latin Hypercube")):
        d = cls(4)
        assert d.get_method() == method
        assert str(d) == method + " Experimental Design with 4 parameters"
    assert issubclass(MaxiMinLHC, LatinHypercubeDesign) and issubclass(LatinHypercubeDesign, ExperimentalDesign)
    assert M.MaxiMinLHC is MaxiMinLHC and M.MonteCarloDesign is MonteCarloDesign and M.LatinHypercubeDesign is LatinHypercubeDesign


def test_sample_checks():
    d = LatinHypercubeDesign(2)
    with pytest.raises(AssertionError):
        d.sample(0)
    with pytest.raises(AssertionError):
        MonteCarloDesign(2, lambda u: np.nan).sample(3)
    with pytest.raises(AssertionError):
        MonteCarloDesign(2, lambda u: np.inf).sample(3)

    class Bad(ExperimentalDesign):
        def _draw_samples(self, n_samples):
            return np.full((n_samples, self.get_n_parameters()), 1.5)
    with pytest.raises(AssertionError):
        Bad(2).sample(3)
    with pytest.raises(AssertionError):
        MaxiMinLHC(2).sample(3, n_tries=0)


# ---- seeded draws against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,tag", [(MonteCarloDesign, "mc"), (LatinHypercubeDesign, "lhc")])
def test_seeded_samples_equal_the_reference(golden, cls, tag):
    g = golden("design.npz")
    cases = oneshot_cases(g, tag)
    assert len(cases) == 5
    for key, name, n, seed in cases:
        np.random.seed(seed)
        got = cls(*DESIGN_ARGS[name]).sample(n)
        assert got.shape == (n, N_PARAMETERS[name])
        assert np.array_equal(got, g[key]), key


def test_latin_hypercube_strata():
    np.random.seed(5)
    n = 37
    s = LatinHypercubeDesign(4)._draw_samples(n)
    for d in range(4):
        assert sorted(np.floor(s[:, d] * n).astype(int)) == list(range(n))


# ---- maximin: selection logic with scipy standing in for the device call ------------------------------------------------------------
def _scipy_scores(calls):
    def fake(designs):
        calls.append(designs.shape)
        return np.array([pdist(d).min() for d in designs])
    return fake


def _pretend_device(monkeypatch, calls):
    monkeypatch.setattr(LibGPGPU, "HAVE_LIBGPGPU", True)
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: True)
    monkeypatch.setattr(LibGPGPU, "design_min_pdist", _scipy_scores(calls), raising=False)


def test_maximin_keeps_the_reference_winner(golden, monkeypatch):
    g = golden("design.npz")
    calls = []
    _pretend_device(monkeypatch, calls)
    cases = [c for c in maximin_cases(g) if c[3] <= 200]
    assert len(cases) == 5
    for key, name, n, n_tries, seed in cases:
        del calls[:]
        np.random.seed(seed)
        got = MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries)
        assert np.array_equal(got, g[key]), key
        assert calls == [(n_tries, n, N_PARAMETERS[name])]          # one device call for all tries
        # the random stream was consumed exactly as the reference consumes it
        np.random.seed(seed)
        for _ in range(n_tries):
            LatinHypercubeDesign(N_PARAMETERS[name])._draw_samples(n)
        after_ref = np.random.random()
        np.random.seed(seed)
        MaxiMinLHC(*DESIGN_ARGS[name])._draw_samples(n, n_tries=n_tries)
        assert np.random.random() == after_ref


def test_maximin_does_not_depend_on_the_chunk(golden, monkeypatch):
    g = golden("design.npz")
    calls = []
    _pretend_device(monkeypatch, calls)
    key, name, n, n_tries, seed = [c for c in maximin_cases(g) if c[1] == "box2"][0]
    monkeypatch.setattr(MaxiMinLHC, "CHUNK_BYTES", 7 * 8 * n * N_PARAMETERS[name])      # seven tries per call
    np.random.seed(seed)
    got = MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries)
    assert np.array_equal(got, g[key])
    assert len(calls) == -(-n_tries // 7) and calls[0][0] == 7


def test_maximin_first_of_equal_tries_wins(monkeypatch):
    monkeypatch.setattr(LibGPGPU, "HAVE_LIBGPGPU", True)
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: True)
    scores = [1., 3., 3., 2., 3.]
    np.random.seed(3)
    tries = [LatinHypercubeDesign(2)._draw_samples(4) for _ in range(5)]
    for tries_per_call in (5, 2, 1):
        served = []

        def fake(designs):
            lo = len(served)
            served.extend(range(lo, lo + len(designs)))
            return np.array(scores[lo:lo + len(designs)])
        monkeypatch.setattr(LibGPGPU, "design_min_pdist", fake, raising=False)
        monkeypatch.setattr(MaxiMinLHC, "CHUNK_BYTES", tries_per_call * 8 * 4 * 2)
        np.random.seed(3)
        got = MaxiMinLHC(2)._draw_samples(4, n_tries=5)
        assert served == list(range(5))
        assert np.array_equal(got, tries[1])


def test_maximin_pdist_keyword_runs_on_the_host(golden, monkeypatch):
    g = golden("design.npz")
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: False)
    key, name, n, n_tries, seed = [c for c in maximin_cases(g) if c[1] == "unit3" and c[3] <= 200][0]
    np.random.seed(seed)
    got = MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries, metric="euclidean")
    assert np.array_equal(got, g[key])
    np.random.seed(seed)
    other = MaxiMinLHC(*DESIGN_ARGS[name]).sample(n, n_tries=n_tries, metric="chebyshev")
    np.random.seed(seed)
    tries = [LatinHypercubeDesign(3)._draw_samples(n) for _ in range(n_tries)]
    best = int(np.argmax([pdist(t, metric="chebyshev").min() for t in tries]))
    assert np.array_equal(other, tries[best])


def test_maximin_without_a_device_raises(monkeypatch):
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: False)
    with pytest.raises(RuntimeError, match="compatible GPU"):
        MaxiMinLHC(2).sample(5)
    monkeypatch.setattr(LibGPGPU, "HAVE_LIBGPGPU", False)
    with pytest.raises(RuntimeError, match="could not be loaded"):
        MaxiMinLHC(2).sample(5)
    # the host-only classes do not care
    assert MonteCarloDesign(2).sample(5).shape == (5, 2)
    assert LatinHypercubeDesign(2).sample(5).shape == (5, 2)


def test_design_min_pdist_argument_checks():
    assert M.HAVE_LIBGPGPU, "libmogp_hip.so did not load: %r" % (LibGPGPU._IMPORT_ERROR,)
    from mogp_emulator_amd import libgpgpu
    with pytest.raises(ValueError):
        libgpgpu.design_min_pdist(np.zeros((3, 1, 2)))               # one point: no pair, as np.min(pdist(...)) raises
    with pytest.raises(TypeError):
        libgpgpu.design_min_pdist(np.zeros((3, 4, 2, 2)))
    with pytest.raises(ValueError):
        libgpgpu.design_min_pdist(np.full((1, 4, 2), np.nan))
    assert "mogp_design_min_pdist" in M._capi.SIGNATURES


# ---- SequentialDesign with a stub metric ----------------------------------------------------------------------------------------------
def _seq():
    from mogp_emulator_amd.SequentialDesign import SequentialDesign
    return SequentialDesign


def _stub(**kw):
    class Stub(_seq()):
        """Always picks the last candidate; the emulator's estimate of a target is 100 + the point's first coordinate."""

        def _eval_metric(self):
            return self.n_cand - 1

        def _estimate_next_target(self, next_point):
            return 100. + next_point[0]
    return Stub(LatinHypercubeDesign(2), **kw)


def f2(x):
    return x[0] + 10. * x[1]


def test_sequential_construction():
    SD = _seq()
    sd = SD(LatinHypercubeDesign(3))
    assert (sd.get_n_parameters(), sd.get_n_init(), sd.get_n_cand(), sd.get_n_samples()) == (3, 10, 50, None)
    assert sd.get_current_iteration() == 0 and not sd.has_function() and not sd.initialized
    assert sd.get_inputs() is None and sd.get_targets() is None and sd.get_candidates() is None
    assert sd.get_base_design() == "LatinHypercubeDesign"
    sd = SD(MonteCarloDesign(1), f=f2, n_samples=7, n_init=3, n_cand=4)
    assert sd.has_function() and sd.get_n_samples() == 7 and sd.get_n_init() == 3 and sd.get_n_cand() == 4
    with pytest.raises(TypeError):
        SD(3)
    with pytest.raises(TypeError):
        SD(LatinHypercubeDesign(2), f=3.)
    with pytest.raises(ValueError):
        SD(LatinHypercubeDesign(2), f=lambda a, b: a)
    with pytest.raises(ValueError):
        SD(LatinHypercubeDesign(2), n_samples=-1)
    with pytest.raises(ValueError):
        SD(LatinHypercubeDesign(2), n_init=0)
    with pytest.raises(ValueError):
        SD(LatinHypercubeDesign(2), n_cand=0)
    with pytest.raises(NotImplementedError):
        sd._eval_metric()
    with pytest.raises(NotImplementedError):
        sd._estimate_next_target(np.zeros(1))


def test_sequential_str():
    sd = _stub(f=f2, n_samples=2, n_init=3, n_cand=4)
    text = str(sd).split("\n")
    assert text[:7] == ["Stub with", "LatinHypercubeDesign base design", "a bound simulator function", "2 total samples",
                        "3 initial points", "4 candidate points", "0 current samples"]
    assert text[7] == "current inputs: None" and text[8] == "current targets: None"
    assert "a bound simulator function" not in str(_stub())


def test_initial_design_and_steps():
    sd = _stub(n_init=4, n_cand=6)
    with pytest.raises(ValueError):
        sd.get_next_point()
    with pytest.raises(ValueError):
        sd.set_initial_targets(np.zeros(4))
    np.random.seed(8)
    X = sd.generate_initial_design()
    assert X.shape == (4, 2) and sd.get_current_iteration() == 4 and sd.get_inputs() is X
    with pytest.raises(ValueError):
        sd.get_next_point()                                  # no targets yet
    with pytest.raises(AssertionError):
        sd.set_initial_targets(np.zeros(3))
    sd.set_initial_targets(np.arange(4.).reshape(4, 1))      # squeezed
    assert sd.get_targets().shape == (4,) and sd.initialized
    with pytest.raises(AssertionError):
        sd.generate_initial_design()
    p = sd.get_next_point()
    assert sd.get_candidates().shape == (6, 2) and np.array_equal(p, sd.get_candidates()[-1])
    assert sd.get_inputs().shape == (5, 2) and np.array_equal(sd.get_inputs()[-1], p) and np.array_equal(sd.get_inputs()[:4], X)
    assert sd.get_current_iteration() == 4 and sd.get_targets().shape == (4,)
    with pytest.raises(AssertionError):
        sd.get_next_point()                                  # the pending point has no target
    with pytest.raises(AssertionError):
        sd.set_next_target([1., 2.])
    sd.set_next_target(np.array([[9.]]))
    assert sd.get_current_iteration() == 5 and np.array_equal(sd.get_targets(), [0., 1., 2., 3., 9.])
    with pytest.raises(AssertionError):
        sd.set_next_target(1.)                               # nothing pending


def test_run_sequential_design_with_a_simulator():
    sd = _stub(f=f2, n_samples=3, n_init=4, n_cand=5)
    np.random.seed(9)
    sd.run_sequential_design()
    assert sd.get_inputs().shape == (7, 2) and sd.get_targets().shape == (7,) and sd.get_current_iteration() == 7
    assert np.array_equal(sd.get_targets(), [f2(x) for x in sd.get_inputs()])
    sd.run_next_point()
    assert sd.get_current_iteration() == 8
    sd2 = _stub(f=f2, n_init=2)
    with pytest.raises(ValueError):
        sd2.run_sequential_design()
    sd2.run_sequential_design(n_samples=0)
    assert sd2.get_current_iteration() == 2
    for method in ("run_initial_design", "run_next_point", "run_sequential_design"):
        with pytest.raises(AssertionError):
            getattr(_stub(), method)()


def test_batch_points_bookkeeping():
    sd = _stub(f=f2, n_init=3, n_cand=4)
    np.random.seed(10)
    sd.run_initial_design()
    t0 = sd.get_targets().copy()
    seen = []
    estimate = sd._estimate_next_target

    def spy(p):
        seen.append((sd.get_current_iteration(), sd.get_targets().copy()))
        return estimate(p)
    sd._estimate_next_target = spy
    with pytest.raises(AssertionError):
        sd.get_batch_points(0)
    batch = sd.get_batch_points(3)
    # kriging believer: every later point was chosen with the earlier ones' ESTIMATED targets in place ...
    assert [it for it, _ in seen] == [3, 4, 5]
    assert np.array_equal(seen[2][1], np.concatenate([t0, 100. + batch[:2, 0]]))
    # ... which are gone afterwards: three inputs wait for their real targets
    assert batch.shape == (3, 2) and np.array_equal(sd.get_inputs()[3:], batch)
    assert sd.get_current_iteration() == 3 and np.array_equal(sd.get_targets(), t0)
    with pytest.raises(AssertionError):
        sd.set_batch_targets([1., 2.])
    sd.set_batch_targets([[1.], [2.], [3.]])
    assert sd.get_current_iteration() == 6 and np.array_equal(sd.get_targets(), np.concatenate([t0, [1., 2., 3.]]))
    sd.get_batch_points(1)
    sd.set_batch_targets(5.)
    assert sd.get_current_iteration() == 7 and sd.get_targets()[-1] == 5.
    with pytest.raises(ValueError):
        _stub().set_batch_targets([1.])


def test_save_and_load(tmp_path):
    sd = _stub(f=f2, n_init=3, n_cand=4)
    np.random.seed(11)
    sd.run_initial_design()
    sd.run_next_point()
    path = str(tmp_path / "design.npz")
    sd.save_design(path)
    back = _stub(n_init=2, n_cand=4)
    back.load_design(path)
    assert np.array_equal(back.get_inputs(), sd.get_inputs()) and np.array_equal(back.get_targets(), sd.get_targets())
    assert np.array_equal(back.get_candidates(), sd.get_candidates())
    assert back.initialized and back.get_current_iteration() == 4
    back.get_next_point()                                    # and the design goes on from there
    assert back.get_inputs().shape == (5, 2)
    # an empty design round-trips as None
    empty = _stub()
    path2 = str(tmp_path / "empty.npz")
    empty.save_design(path2)
    back = _stub()
    back.load_design(path2)
    assert back.get_inputs() is None and back.get_targets() is None and back.get_candidates() is None and not back.initialized
    # inputs without targets (a generated, not yet evaluated initial design)
    fresh = _stub(n_init=2)
    fresh.generate_initial_design()
    path3 = str(tmp_path / "fresh.npz")
    fresh.save_design(path3)
    back = _stub(n_init=2)
    back.load_design(path3)
    assert back.get_inputs().shape == (2, 2) and back.get_targets() is None and not back.initialized
    wrong = type(back)(LatinHypercubeDesign(3))
    with pytest.raises(AssertionError):
        wrong.load_design(path)


def test_load_design_shrinks_n_init_to_the_saved_points(tmp_path, capsys):
    """n_init follows the number of saved POINTS when there are fewer of them; the number of parameters has no say (the reference
    compares the parameters here, which is not mirrored)."""
    sd = _stub(f=f2, n_init=5, n_cand=4)
    np.random.seed(12)
    sd.run_initial_design()
    path = str(tmp_path / "five.npz")
    sd.save_design(path)
    same = _stub(n_init=5, n_cand=4)                       # 5 points of 2 parameters: nothing to change
    same.load_design(path)
    assert same.get_n_init() == 5 and "changing n_init" not in capsys.readouterr().out
    more = _stub(n_init=8, n_cand=4)
    more.load_design(path)
    assert more.get_n_init() == 5 and "changing n_init" in capsys.readouterr().out
    assert more.get_current_iteration() == 5


def test_mice_step_without_a_device_raises_at_once(monkeypatch):
    assert M.HAVE_LIBGPGPU, "libmogp_hip.so did not load: %r" % (LibGPGPU._IMPORT_ERROR,)
    from mogp_emulator_amd.SequentialDesign import MICEDesign
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: False)
    md = MICEDesign(LatinHypercubeDesign(2), f=f2, n_init=4, n_cand=5)
    md.run_initial_design()
    with pytest.raises(RuntimeError, match="compatible GPU"):
        md.get_next_point()


def test_mice_design_construction():
    assert M.HAVE_LIBGPGPU, "libmogp_hip.so did not load: %r" % (LibGPGPU._IMPORT_ERROR,)
    from mogp_emulator_amd.SequentialDesign import MICEDesign, SequentialDesign
    assert M.MICEDesign is MICEDesign and M.SequentialDesign is SequentialDesign and issubclass(MICEDesign, SequentialDesign)
    md = MICEDesign(LatinHypercubeDesign(2))
    assert md.get_nugget() == "adaptive" and md.get_nugget_s() == 1. and md.get_n_cand() == 50
    md = MICEDesign(LatinHypercubeDesign(2), f=f2, n_samples=3, n_init=5, n_cand=200, nugget=1.e-6, nugget_s=2)
    assert md.get_nugget() == 1.e-6 and md.get_nugget_s() == 2. and isinstance(md.get_nugget_s(), float) and md.get_n_cand() == 200
    assert str(md).startswith("MICEDesign with\nLatinHypercubeDesign base design\n")
    with pytest.raises(ValueError):
        MICEDesign(LatinHypercubeDesign(2), nugget=-1.)
    with pytest.raises(ValueError):
        MICEDesign(LatinHypercubeDesign(2), nugget_s=-1.)
    with pytest.raises(TypeError):
        MICEDesign(LatinHypercubeDesign(2), nugget=[1., 2.])
    with pytest.raises(TypeError):
        MICEDesign(3)
    with pytest.raises(AssertionError):
        md._MICE_criterion(200)
