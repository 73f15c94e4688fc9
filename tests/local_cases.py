"""The shapes of the local-prediction tests (test_local_host.py, test_gpu_local.py) and their restatement values, computed once per
process and shared.  Inputs come from dimension_cases.case (its theta rule and NUGGET); plain NumPy, nothing here touches the device."""
import functools

import numpy as np

import dimension_cases as dc
import local_restate as lr

KERNELS = ["SquaredExponential", "Matern52", "UniformSqExp", "UniformMat52"]
SHAPES = [(300, 3, 8), (300, 3, 50), (300, 3, 126), (1000, 5, 64), (130, 17, 126), (126, 2, 126)]      # (N, D, k)
M = 37
D_ENDS_AND_EDGES = [1] + dc.D_EDGES[:-1] + [79, 80]        # 1, 16, 17, 32, 33, 79, 80
SWEEP_K = 16
SWEEP_KERNELS = KERNELS[:2]                                  # the per-dimension kernels
# odd k: the tile's k + 2 rows are an odd count, whose middle row is its own partner in the kernel's mirrored row pairs; k = 1 is the least
ODD_K = [(130, 3, 1), (130, 3, 7), (130, 3, 125)]
ALL = ([(N, D, k, kern) for (N, D, k) in SHAPES for kern in KERNELS] + [(dc.N_TILES, D, SWEEP_K, kern) for D in D_ENDS_AND_EDGES
                                                                        for kern in SWEEP_KERNELS]
       + [(N, D, k, kern) for (N, D, k) in ODD_K for kern in SWEEP_KERNELS])
SIGMA2 = float(np.exp(dc.LOG_COV))


@functools.lru_cache(maxsize=None)
def setup(N, D, kernel, E=1):
    """(case, [scales of emulator e])"""
    c = dc.case(N, D, kernel, m=M, E=E)
    return c, [lr.scales(c.thetas[e][:c.nc], D, kernel) for e in range(E)]


@functools.lru_cache(maxsize=None)
def reference(N, D, k, kernel):
    """the restatement on its own neighbour lists, float64: dict(nbr, radius, r2, mean, var, cond)"""
    c, (s,) = setup(N, D, kernel)
    nbr, radius, r2 = lr.neighbours(c.X, c.Xs, s, k)
    mean, var, ok, cond = lr.predict(c.X, c.T[0], c.Xs, s, kernel, SIGMA2, dc.NUGGET, nbr)
    assert ok.all()
    return dict(nbr=nbr, radius=radius, r2=r2, mean=mean, var=var, cond=cond)


def excess_rows(tag, got, want, cond):
    """dimension_cases.excess row by row, every row at the amplification of its own local matrix"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape == np.shape(cond), (tag, got.shape, want.shape)
    return max(dc.excess(tag, got[j:j + 1], want[j:j + 1], max(1., float(cond[j]) * 1e-7)) for j in range(got.shape[0]))
