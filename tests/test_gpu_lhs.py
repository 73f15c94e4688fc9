"""The Latin-hypercube annealer on the MI355X against its NumPy restatement (lhs_restate.py): levels, accepted counts, min R and pair
counts equal, Phi equal bit for bit, at the shapes where the kernel takes another path (no third row, less than a wave, one past a wave,
one past the workgroup, the widest row, both level widths, more chains than CUs); and OptimisedLHC on top of it."""
import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd.ExperimentalDesign import MaxiMinLHC, OptimisedLHC

import lhs_restate as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def starts(seed, C, n, D):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(n) for _ in range(D)], axis=1) for _ in range(C)])


def assert_same(got, want, what):
    assert np.array_equal(got.levels, want["levels"]), what + ": levels"
    assert np.array_equal(got.accepted, want["accepted"]), what + ": accepted"
    assert np.array_equal(got.min_r, want["min_r"]) and np.array_equal(got.pairs, want["pairs"]), what + ": min R / pairs"
    assert got.phi.tobytes() == want["phi"].tobytes(), what + ": Phi"


# (n, D, chains, proposals, q)
EQUALITY_CASES = [(2, 1, 1, 300, 5), (3, 2, 5, 500, 1), (8, 2, 5, 2000, 5), (65, 3, 5, 1000, 5), (65, 3, 1, 1000, 1), (257, 4, 5, 600, 5),
                  (257, 4, 1, 600, 1), (300, 80, 1, 300, 5), (1100, 2, 1, 200, 5), (65536, 1, 1, 200, 5), (70000, 1, 1, 200, 5), (8, 2, 300, 300, 5),
                  (65, 3, 300, 200, 1)]


@pytest.mark.parametrize("n,D,C,steps,q", EQUALITY_CASES)
def test_device_equals_the_restatement(n, D, C, steps, q):
    from mogp_emulator_amd import libgpgpu
    S = starts(1009 * n + D, C, n, D)
    kw = dict(q=q, theta0=0.1, rho=0.9, seed=2 ** 40 + 12345 + n, stream=2 ** 32 - 2)        # the stream wraps within the call
    got = libgpgpu.design_anneal_lhs(S, steps, **kw)
    want = lr.anneal(S, steps, **kw)
    print("n=%d D=%d C=%d q=%d: accepted %s, min R %s" % (n, D, C, q, got.accepted[:5].tolist(), got.min_r[:5].tolist()))
    assert got.levels.dtype == np.int32 and got.levels.shape == (C, n, D)
    assert_same(got, want, "n=%d D=%d" % (n, D))
    if D > 1 and n > 2:             # (with one column Phi is the same for every design: Delta is rounding noise, all is accepted)
        assert np.any(got.accepted > 0) and np.any(got.accepted < steps)         # both branches of the decision ran


def test_other_schedules_and_no_steps():
    from mogp_emulator_amd import libgpgpu
    S = starts(5, 3, 40, 3)
    for kw in (dict(theta0=0., rho=1., stage=1), dict(theta0=0.5, rho=0.5, stage=7), dict(theta0=0.1, rho=0.9, stage=10 ** 12)):
        assert_same(libgpgpu.design_anneal_lhs(S, 400, seed=3, **kw), lr.anneal(S, 400, seed=3, **kw), str(kw))
    got = libgpgpu.design_anneal_lhs(S, 0)
    assert np.array_equal(got.levels, S) and np.all(got.accepted == 0)
    assert_same(got, lr.anneal(S, 0), "no steps")


def test_chain_of_a_batch_equals_the_single_call_and_repeats():
    from mogp_emulator_amd import libgpgpu
    S = starts(6, 5, 65, 3)
    a = libgpgpu.design_anneal_lhs(S, 800, seed=9, stream=4)
    b = libgpgpu.design_anneal_lhs(S, 800, seed=9, stream=4)
    for key in ("levels", "phi", "min_r", "pairs", "accepted"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    for c in (0, 3, 4):
        one = libgpgpu.design_anneal_lhs(S[c], 800, seed=9, stream=4 + c)
        for key in ("levels", "phi", "min_r", "pairs", "accepted"):
            assert np.array_equal(getattr(one, key)[0], getattr(a, key)[c]), key
    assert not np.array_equal(libgpgpu.design_anneal_lhs(S, 800, seed=10, stream=4).levels, a.levels)


def test_refusals_come_without_a_launch():
    from mogp_emulator_amd import libgpgpu
    with pytest.raises(RuntimeError, match="does not fit the LDS"):
        libgpgpu.design_anneal_lhs(np.tile(np.arange(37633)[None, :, None], (1, 1, 2)), 10)
    bad = starts(1, 2, 10, 2)
    bad[1, 3, 0] = bad[1, 4, 0]
    with pytest.raises(RuntimeError, match="column 0 of start 1 is not a permutation"):
        libgpgpu.design_anneal_lhs(bad, 10)


# ---- OptimisedLHC -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", ["centre", "random"])
def test_sample_is_a_latin_hypercube(offsets):
    n, D = 37, 4
    np.random.seed(11)
    X = OptimisedLHC(D).sample(n, n_chains=6, n_steps=2000, offsets=offsets)
    assert X.shape == (n, D) and np.all((X >= 0.) & (X <= 1.))
    assert np.array_equal(np.sort(np.floor(X * n).astype(int), axis=0), np.tile(np.arange(n)[:, None], (1, D)))
    if offsets == "centre":
        assert np.array_equal(X, (np.floor(X * n) + 0.5) / n)
    np.random.seed(11)
    assert np.array_equal(OptimisedLHC(D).sample(n, n_chains=6, n_steps=2000, offsets=offsets), X)
    np.random.seed(12)
    assert not np.array_equal(OptimisedLHC(D).sample(n, n_chains=6, n_steps=2000, offsets=offsets), X)


def test_bounds_ppf_start_and_info():
    np.random.seed(4)
    ed = OptimisedLHC([(0., 2.), (-3., 5.), lambda u: 10. * u])
    X, info = ed.sample(20, n_chains=9, n_steps=1500, return_info=True)
    assert X.shape == (20, 3) and np.all(X[:, 0] <= 2.) and X[:, 1].min() < 0. and X[:, 2].max() > 5.
    assert info["winner"] == lr.winner(info["min_r"], info["pairs"]) and len(info["phi"]) == 9
    lev = np.stack([np.floor(X[:, 0] / 2. * 20), np.floor((X[:, 1] + 3.) / 8. * 20), np.floor(X[:, 2] / 10. * 20)], axis=1).astype(int)
    assert lr.criteria(lev) == (info["min_r"][info["winner"]], info["pairs"][info["winner"]])
    # the tie rule on equal chains: the same start three times under one stream each is three different chains; no steps makes them equal
    S = np.repeat(lev[None], 3, axis=0)
    X0, info0 = OptimisedLHC(3).sample(20, start=S, n_steps=0, return_info=True)
    assert info0["winner"] == 0 and np.array_equal(X0, (lev + 0.5) / 20.)
    # polishing a design: never worse than the start
    X1, info1 = OptimisedLHC(3).sample(20, start=lev, n_steps=500, seed=1, return_info=True)
    assert info1["phi"][0] <= info["phi"][info["winner"]] and len(info1["phi"]) == 1


def test_beats_maximin_at_30_by_3():
    from mogp_emulator_amd import libgpgpu
    np.random.seed(2024)
    opt = OptimisedLHC(3).sample(30)
    np.random.seed(2024)
    rnd = MaxiMinLHC(3).sample(30, n_tries=1000)
    d_opt, d_rnd = libgpgpu.design_min_pdist(opt)[0], libgpgpu.design_min_pdist(rnd)[0]
    print("minimum distance at n = 30, D = 3: OptimisedLHC %.4f, MaxiMinLHC of 1000 tries %.4f" % (d_opt, d_rnd))
    assert d_opt > d_rnd


def test_base_design_of_mice():
    from mogp_emulator_amd import MICEDesign
    np.random.seed(1)
    md = MICEDesign(OptimisedLHC(2, (0., 2.)), f=lambda x: np.sin(3. * x[0]) + x[1] * x[1], n_samples=1, n_init=8, n_cand=20, nugget=1.e-6)
    md.run_initial_design()
    X = md.get_inputs()
    assert X.shape == (8, 2) and np.all((X >= 0.) & (X <= 2.)) and md.get_base_design() == "OptimisedLHC"
    assert np.array_equal(np.sort(np.floor(X / 2. * 8).astype(int), axis=0), np.tile(np.arange(8)[:, None], (1, 2)))
