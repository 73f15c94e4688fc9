"""Pathwise posterior draws past one block of 1024 rows, on the MI355X: N = 1030 with 130 features (three tiles, the last partial) and 17
draws (two MFMA blocks, the second partial), so that the right-hand sides, the dots of the solve and the feature product at the design all
run a second, partial block.  The conditioning identity alone (test_gpu_pathwise.conditioning_check): f_s(X) + eta v_s + sqrt(eta) eps_s
reproduces y up to A v_s - b_s, whose norm the reported residual and the bars of the two products account for.  test_pathwise_host.py
shows on the CPU that the restatement's solver converges on these right-hand sides within 600 iterations; 1000 are allowed here."""
import numpy as np
import pytest

import large_design_cases as ld
import test_gpu_iterative as tg
import test_gpu_pathwise as tp
import test_pathwise_host as ph
from test_iterative_host import MAX_ITER

pytestmark = pytest.mark.gpu


def test_paths_reproduce_the_data_at_a_design_of_two_blocks():
    n, D, kernel, p = ld.ITER_SOLVE_SHAPES[0]
    assert n == 1030
    F, S = 130, 17
    c, s, ig = tg._iter(n, D, kernel, p)
    W, eps = ph.path_normals(n, S, F, seed=6)
    paths = ig.sample_paths(S, n_features=F, feature_normals=W, noise_normals=eps)
    assert paths.update.shape == (n, S) and paths.converged.all() and paths.iterations.max() <= MAX_ITER
    worst = tp.conditioning_check(c, s, kernel, ig, c.T[0], paths, eps)
    ig.close()
    print("n %d D %d %s F %d S %d: conditioning identity at %.3g of what the residual and the products allow" % (n, D, kernel, F, S, worst))
    assert worst <= 1.
    assert np.all(np.isfinite(paths.update))
