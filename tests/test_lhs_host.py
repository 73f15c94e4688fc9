"""Host-side checks of the Latin-hypercube annealer: the NumPy restatement (lhs_restate.py, which the device is held to in
test_gpu_lhs.py) keeps permutations, is accurate, improves on its start, reaches the enumerated optimum at n = 8, D = 2 and beats 1000
random hypercubes at n = 30, D = 3; the limits header (csrc/lhs_plan.h) through a sanitised host program; the refusals that need no
device."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.ExperimentalDesign import LatinHypercubeDesign, OptimisedLHC

import lhs_restate as lr
import sample_restate as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def starts(seed, C, n, D):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(n) for _ in range(D)], axis=1) for _ in range(C)])


def is_lhs(P):
    n = P.shape[-2]
    return bool(np.all(np.sort(P, axis=-2) == np.arange(n).reshape((n, 1))))


@pytest.fixture(scope="module")
def run_30_3():
    S = starts(30, 4, 30, 3)
    return S, lr.anneal(S, 20000, q=5, seed=12)


def test_philox_block_is_the_known_one():
    for ctr, key, want in sr.KAT:
        got = lr.philox_block(*[np.array([c]) for c in ctr], key[0], key[1])
        assert tuple(int(w[0]) for w in got) == want
    d, a, b, u = lr.proposal(5, np.arange(4000), 99, 7, 3)
    assert d.min() >= 0 and d.max() <= 2 and a.min() >= 0 and a.max() <= 6 and b.min() >= 0 and b.max() <= 6
    assert np.all(a != b) and np.all((u >= 0.) & (u < 1.))
    assert set(np.unique(b)) == set(range(7))
    # a counter above 2^32 uses the high word
    assert lr.proposal(2 ** 32 + 5, [0], 99, 7, 3) != lr.proposal(5, [0], 99, 7, 3)


def test_every_column_stays_a_permutation(run_30_3):
    S, r = run_30_3
    assert is_lhs(r["levels"])
    for n, D, steps in ((2, 1, 50), (3, 2, 200), (65, 3, 300), (257, 4, 100)):
        out = lr.anneal(starts(n, 2, n, D), steps, seed=n)
        assert is_lhs(out["levels"]) and out["levels"].shape == (2, n, D)


def test_phi_against_long_double(run_30_3):
    """Bound: 2 q u relative, u = 2^-53.  g(R) takes q - 1 rounded multiplications and one rounded division, so every term is within
    q u (1 + q u) < 2 q u of the exact one, and a sum of positive terms is no further from the exact sum, relatively, than its worst term.
    The additions of the double sum round too (each multiplies the partial sum by 1 + e, |e| <= u); the factor 2 is the room for them.
    Every term is held to 2 q u on its own, and Phi is held to 2 q u as well."""
    S, r = run_30_3
    for P, q in ((r["levels"][0], 5), (S[1], 5), (starts(7, 1, 65, 3)[0], 1), (starts(8, 1, 257, 4)[0], 3)):
        P = P.astype(np.int64)
        iu = np.triu_indices(len(P), 1)
        R = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)[iu]
        exact = 1.0 / R.astype(np.longdouble) ** q
        assert np.max(np.abs(lr.g(R, q).astype(np.longdouble) - exact) / exact) <= 2 * q * U
        want = exact.sum()
        got = lr.phi(P, q)
        rel = abs(np.longdouble(got) - want) / want
        print("n = %d, q = %d: Phi off by %.3g relative (bound %.3g)" % (len(P), q, rel, 2 * q * U))
        assert rel <= 2 * q * U


def test_one_column_shortcuts_equal_the_general_code():
    for n, q in ((2, 5), (3, 1), (300, 5), (300, 1)):
        P = starts(n, 1, n, 1)[0]
        assert np.array_equal(lr.row_sums_general(P, q), lr.row_sums_one_column(n, q))
        R = (P[:, None, 0] - P[None, :, 0]) ** 2
        R = R[np.triu_indices(n, 1)]
        assert lr.criteria(P) == (int(R.min()), int((R == R.min()).sum()))


def test_best_is_no_worse_than_the_start(run_30_3):
    S, r = run_30_3
    for c in range(len(S)):
        assert r["phi"][c] <= lr.phi(S[c], 5)
        assert r["accepted"][c] > 0


def test_chains_are_independent():
    S = starts(3, 3, 9, 2)
    all3 = lr.anneal(S, 400, seed=5, stream=7)
    for c in range(3):
        one = lr.anneal(S[c], 400, seed=5, stream=7 + c)
        for key in ("levels", "phi", "min_r", "pairs", "accepted", "phi_run"):
            assert np.array_equal(all3[key][c], one[key][0]), key
    assert not np.array_equal(all3["levels"][0], lr.anneal(S[0], 400, seed=6, stream=7)["levels"][0])


def test_no_steps_is_the_identity():
    S = starts(4, 2, 12, 3)
    r = lr.anneal(S, 0)
    assert np.array_equal(r["levels"], S) and np.all(r["accepted"] == 0)
    for c in range(2):
        assert r["phi"][c] == lr.phi(S[c], 5) and (r["min_r"][c], r["pairs"][c]) == lr.criteria(S[c])


def test_two_points_accept_everything():
    r = lr.anneal(starts(2, 1, 2, 1), 30)
    assert r["accepted"][0] == 30 and r["phi"][0] == 1.0 and (r["min_r"][0], r["pairs"][0]) == (1, 1)


def test_reaches_the_enumerated_optimum_at_8_by_2():
    base = np.arange(8)
    iu = np.triu_indices(8, 1)
    optimum = 0
    for perm in itertools.permutations(range(8)):
        p = np.array(perm)
        optimum = max(optimum, int(((base[:, None] - base[None, :]) ** 2 + (p[:, None] - p[None, :]) ** 2)[iu].min()))
    assert optimum == 8
    r = lr.anneal(starts(8, 8, 8, 2), 2000, seed=11)
    w = lr.winner(r["min_r"], r["pairs"])
    print("n = 8, D = 2: min R of the chains", r["min_r"].tolist())
    assert r["min_r"][w] == optimum


def test_beats_a_thousand_random_hypercubes_at_30_by_3(run_30_3):
    S, r = run_30_3
    rnd = starts(1000, 1000, 30, 3)
    best_random = max(lr.criteria(P)[0] for P in rnd)
    w = lr.winner(r["min_r"], r["pairs"])
    print("n = 30, D = 3: chains", r["min_r"].tolist(), "best of 1000 random hypercubes", best_random)
    assert r["min_r"][w] > best_random


def test_winner_rule():
    assert lr.winner([5, 9, 9, 9], [1, 4, 2, 2]) == 2
    res = LibGPGPU.AnnealResult(None, None, np.array([5, 9, 9, 9]), np.array([1, 4, 2, 2]), None) if M.HAVE_LIBGPGPU else None
    assert res is None or res.winner == 2


def test_limits_header(tmp_path):
    """tests/c/lhs_plan_check.cpp checks csrc/lhs_plan.h against the documented formulas (sanitised build); its edge and overflow lines
    against this module's own restatement of them"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "lhs_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", "lhs_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "cases ok" in out.stdout, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    edges = {ln[1]: [int(v) for v in ln[2:]] for ln in lines if ln[0] == "edge"}
    # largest accepted / first refused n D for both widths: 2 n D <= 160 KiB - 13 KiB;  (2 + 1/8) * ceil32(n D) <= the same
    narrow, wide = (160 * 1024 - 13 * 1024) // 2, (160 * 1024 - 13 * 1024) * 8 // 17 // 32 * 32
    assert edges == {"narrow": [narrow, 1, 0], "wide": [wide, 1, 0]}
    assert lr.fits(narrow // 2, 2) and not lr.fits(narrow // 2 + 1, 2) and lr.fits(wide, 1) and not lr.fits(wide + 1, 1)
    assert lr.fits(2000, 10) and lr.fits(5000, 10) and lr.fits(70000, 1) and lr.lds_bytes(70000, 1) == (True, 148784)
    pows = [[int(v) for v in ln[1:]] for ln in lines if ln[0] == "pow"]
    assert len(pows) == 40
    for q, a, b in pows:
        assert bool(a) == lr.power_overflows(2000, 10, q) and bool(b) == lr.power_overflows(70000, 1, q)


def test_python_refusals_without_a_device(monkeypatch):
    assert M.OptimisedLHC is OptimisedLHC and issubclass(OptimisedLHC, LatinHypercubeDesign)
    ed = OptimisedLHC(3)
    assert ed.get_method() == "Latin Hypercube" and ed.get_n_parameters() == 3
    with pytest.raises(ValueError, match="offsets"):
        ed.sample(5, offsets="corner")
    monkeypatch.setattr(LibGPGPU, "HAVE_LIBGPGPU", False)
    with pytest.raises(RuntimeError, match="could not be loaded"):
        ed.sample(5)
    monkeypatch.setattr(LibGPGPU, "HAVE_LIBGPGPU", True)
    monkeypatch.setattr(LibGPGPU, "gpu_usable", lambda: False)
    with pytest.raises(RuntimeError, match="compatible GPU could not be found"):
        ed.sample(5)


@pytest.mark.skipif(not M.HAVE_LIBGPGPU, reason="library not built")
def test_library_refusals_without_a_device():
    """everything the library checks comes before its first device call"""
    from mogp_emulator_amd import libgpgpu
    assert "mogp_design_anneal_lhs" in M._capi.SIGNATURES and "design_anneal_lhs" in libgpgpu.__all__
    ok = starts(1, 1, 6, 2)
    with pytest.raises(TypeError):
        libgpgpu.design_anneal_lhs(ok.astype(float), 10)
    with pytest.raises(TypeError):
        libgpgpu.design_anneal_lhs(ok[0, :, 0], 10)
    bad = ok.copy()
    bad[0, 0, 1] = bad[0, 1, 1]
    with pytest.raises(RuntimeError, match="column 1 of start 0 is not a permutation"):
        libgpgpu.design_anneal_lhs(bad, 10)
    with pytest.raises(RuntimeError, match="does not fit the LDS"):
        libgpgpu.design_anneal_lhs(np.tile(np.arange(37633)[None, :, None], (1, 1, 2)), 10)
    with pytest.raises(RuntimeError, match="does not fit the LDS"):
        libgpgpu.design_anneal_lhs(np.arange(70817)[None, :, None], 10)
    with pytest.raises(RuntimeError, match="reaches 2\\^1000"):
        libgpgpu.design_anneal_lhs(np.arange(3000)[None, :, None], 10, q=44)
    for kw, word in ((dict(q=0), "q must"), (dict(rho=0.), "rho"), (dict(rho=1.5), "rho"), (dict(theta0=-1.), "theta0"),
                     (dict(stage=0), "stage"), (dict(theta0=float("nan")), "theta0")):
        with pytest.raises(RuntimeError, match=word):
            libgpgpu.design_anneal_lhs(ok, 10, **kw)
    with pytest.raises(RuntimeError, match="n_steps"):
        libgpgpu.design_anneal_lhs(ok, -1)
    with pytest.raises(RuntimeError, match="dimensions"):
        libgpgpu.design_anneal_lhs(np.tile(np.arange(4)[None, :, None], (1, 1, 81)), 10)
    with pytest.raises(RuntimeError, match="two points"):
        libgpgpu.design_anneal_lhs(np.zeros((1, 1, 2), dtype=int), 10)
