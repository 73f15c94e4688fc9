"""The estimators of the sensitivity analysis, pinned on the host: the NumPy restatement (sobol_restate.py) that the device results are
compared with reproduces the analytic Sobol indices of the Ishigami function, and pick-freeze builds AB_i as defined."""
import numpy as np
from numpy.testing import assert_allclose

from sobol_restate import all_points, ishigami, ishigami_exact, pick_freeze, sobol_restate, split_points


def test_restatement_gives_the_ishigami_indices():
    """a = 7, b = 0.1, inputs uniform on [-pi, pi]^3, RandomState(0), N = 65 536: S = (0.3139, 0.4424, 0), ST = (0.5576, 0.4424,
    0.2437) within 0.02 absolute (over 20 seeds the worst deviations were 0.009 for S and 0.0103 for ST; the bound is twice that)."""
    rs = np.random.RandomState(0)
    N, D = 65536, 3
    A = rs.uniform(-np.pi, np.pi, (N, D))
    B = rs.uniform(-np.pi, np.pi, (N, D))
    fAB = np.stack([ishigami(pick_freeze(A, B, i)) for i in range(D)])
    r = sobol_restate(ishigami(A), ishigami(B), fAB)
    print("S", r["first_order"], "ST", r["total"], "mean", r["mean"], "variance", r["variance"])
    assert_allclose(r["first_order"], [0.3139, 0.4424, 0.], rtol=0, atol=0.02)
    assert_allclose(r["total"], [0.5576, 0.4424, 0.2437], rtol=0, atol=0.02)
    # the quoted figures are the analytic ones
    S, ST = ishigami_exact()
    assert_allclose(S, [0.3139, 0.4424, 0.], atol=5e-5)
    assert_allclose(ST, [0.5576, 0.4424, 0.2437], atol=5e-5)
    assert_allclose(r["mean"], 3.5, atol=0.05)                                      # a / 2
    assert_allclose(r["variance"], 49. / 8 + 0.1 * np.pi ** 4 / 5 + 0.01 * np.pi ** 8 / 18 + 0.5, rtol=0.02)


def test_restatement_batches_over_leading_axes_and_handles_a_constant():
    rs = np.random.RandomState(1)
    N, D = 512, 3
    A, B = rs.uniform(-np.pi, np.pi, (N, D)), rs.uniform(-np.pi, np.pi, (N, D))
    f = np.stack([ishigami(all_points(A, B)), np.full((D + 2) * N, 2.5), all_points(A, B)[:, 1] * 3.])
    fA, fB, fAB = split_points(f, N, D)
    r = sobol_restate(fA, fB, fAB)
    assert r["first_order"].shape == (3, D) and r["mean"].shape == (3,)
    one = sobol_restate(fA[0], fB[0], fAB[0])
    assert np.array_equal(one["first_order"], r["first_order"][0]) and np.array_equal(one["total"], r["total"][0])
    # a constant: variance exactly 0, NaN indices, no exception
    assert r["variance"][1] == 0. and r["mean"][1] == 2.5
    assert np.all(np.isnan(r["first_order"][1])) and np.all(np.isnan(r["total"][1]))
    # a function of one input alone: its total effect is 1, the others' indices are exactly 0
    assert_allclose(r["total"][2], [0., 1., 0.], atol=0.1)
    assert r["total"][2][0] == 0. and r["total"][2][2] == 0. and r["first_order"][2][0] == 0.


def test_pick_freeze_is_a_with_one_column_of_b():
    rs = np.random.RandomState(2)
    A, B = rs.normal(size=(37, 5)), rs.normal(size=(37, 5))
    for i in range(5):
        AB = pick_freeze(A, B, i)
        assert AB.shape == A.shape
        for d in range(5):
            assert np.array_equal(AB[:, d], (B if d == i else A)[:, d])
    assert np.array_equal(A, np.asarray(A)) and pick_freeze(A, B, 0) is not A          # A itself is untouched
    P = all_points(A, B)
    assert P.shape == (7 * 37, 5)
    assert np.array_equal(P[:37], A) and np.array_equal(P[37:74], B) and np.array_equal(P[74 + 3 * 37:74 + 4 * 37], pick_freeze(A, B, 3))
    fA, fB, fAB = split_points(P[:, 2], 37, 5)
    assert np.array_equal(fA, A[:, 2]) and np.array_equal(fB, B[:, 2])
    assert np.array_equal(fAB[2], B[:, 2]) and np.array_equal(fAB[1], A[:, 2])
