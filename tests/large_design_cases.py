"""The shapes and inputs of the large-design tests (test_large_design_host.py, test_gpu_large_design.py): the smallest at which the
large-design kernels split their work -- a persistent grid whose workgroups take a second and a third problem, a second block of 1024 rows
in the dots, the argmax and the Vecchia sum, a second segment of 4096 rows in the preconditioner's L^T R.  Plain NumPy: nothing here touches
the device.

The grid is LOCAL_GRID_PER_CU workgroups per compute unit (csrc/predict_plan.h, pinned on the host by tests/c/local_plan_check.cpp); the GPU
tests read the compute-unit count of the device they run on, the host tests take HOST_CUS.  Hyperparameters are those of
dimension_cases.case: fixed nugget 1e-4 (0 in the failure designs), sigma^2 = e^0.1."""
import functools

import numpy as np

import dimension_cases as dc
import iterative_restate as ir
import local_restate as lr
import vecchia_cases as vc
import vecchia_restate as vr

LOCAL_GRID_PER_CU = 4
HOST_CUS = 256                       # an MI355X: the host tests show the references' conditions at the grid of 1024
SIGMA2 = float(np.exp(dc.LOG_COV))
FAR = 10.                            # the shift of the far region in coordinate 0: beyond every clean point in every metric used here

DOT_BLOCK, SEG = 1024, 4096          # ITER_DOT_BLOCK (the argmax and VECCHIA_REDUCE_BLOCK are 1024 too) and ITER_SEG


def grid_of(cus):
    cus = int(cus)
    assert cus >= 1, "the compute-unit count of the device could not be read"
    return LOCAL_GRID_PER_CU * cus


# ---- A. LocalGP ----------------------------------------------------------------------------------------------------------------------------
LOCAL = dict(N=300, D=3, k=50)
LOCAL_KERNELS = ["Matern52", "SquaredExponential"]
LOCAL_FAIL_KERNEL = "Matern52"       # without a nugget its clean local matrices stay well conditioned (the host test asserts it)


def local_m(grid):
    return 2 * grid + 37             # every workgroup takes two problems, 37 take three


def local_singles(grid):
    return (0, grid, grid + 5, 2 * grid + 36)


@functools.lru_cache(maxsize=None)
def local_setup(kernel, grid):
    c = dc.case(LOCAL["N"], LOCAL["D"], kernel, m=local_m(grid))
    return c, lr.scales(c.thetas[0][:c.nc], LOCAL["D"], kernel)


@functools.lru_cache(maxsize=None)
def local_reference(kernel, grid):
    """the restatement on its own lists, all 2 grid + 37 rows: dict(nbr, radius, mean, var, cond)"""
    c, s = local_setup(kernel, grid)
    nbr, radius, _ = lr.neighbours(c.X, c.Xs, s, LOCAL["k"])
    mean, var, ok, cond = lr.predict(c.X, c.T[0], c.Xs, s, kernel, SIGMA2, dc.NUGGET, nbr)
    assert ok.all()
    return dict(nbr=nbr, radius=radius, mean=mean, var=var, cond=cond)


@functools.lru_cache(maxsize=None)
def local_failure(grid):
    """(X, t, Q, s, n_far): 300 clean points, then 150 points of the far region present twice (nugget 0: their local matrices are exactly
    singular); the first `grid` queries lie in the far region, the following grid + 37 in the clean one"""
    c, s = local_setup(LOCAL_FAIL_KERNEL, grid)
    far = c.X[:150].copy()
    far[:, 0] += FAR
    X = np.concatenate([c.X, far, far])
    t = np.concatenate([c.T[0], c.T[0, :150], c.T[0, :150]])
    Q = c.Xs.copy()
    Q[:grid, 0] += FAR
    return X, t, Q, s, grid


# ---- B. Vecchia ----------------------------------------------------------------------------------------------------------------------------
VECCHIA = dict(D=3, k=30)
VECCHIA_CASES = [("Matern52", True), ("SquaredExponential", False)]       # (kernel, nugget fitted), random order
VECCHIA_FAIL_KERNEL = "Matern52"
VECCHIA_CLEAN_HEAD, VECCHIA_FAR_POINTS = 100, 300


def vecchia_n(grid):
    n = 2 * grid + 52
    assert n > grid and n > DOT_BLOCK, "N must exceed both the grid and one block of the sum"
    return n


def vecchia_launches(grid):
    return (grid, 512, 7 * 64 + 1)


def vecchia_reference(kernel, fit, grid):
    """vecchia_cases.reference at N = 2 grid + 52 (cached there)"""
    return vc.reference(vecchia_n(grid), VECCHIA["D"], VECCHIA["k"], kernel, fit)


@functools.lru_cache(maxsize=None)
def vecchia_failure(grid):
    """(X, t, theta, s, sigma2, clean (N,) bool) in identity order: positions 0 .. 99 clean, then 300 far points and their 300 copies, then
    clean points up to N = 2 grid + 52.  Every copy has its original among its neighbours: with nugget 0 its matrix is exactly singular."""
    N = vecchia_n(grid)
    head, nf = VECCHIA_CLEAN_HEAD, VECCHIA_FAR_POINTS
    assert N >= head + 2 * nf + grid, "the clean tail must reach one grid behind the far region"
    c, theta, s, sigma2, _ = vc.setup(N, VECCHIA["D"], VECCHIA_FAIL_KERNEL, False)
    X = c.X.copy()
    far = X[head:head + nf].copy()
    far[:, 0] += FAR
    X[head:head + nf] = far
    X[head + nf:head + 2 * nf] = far
    t = c.T[0].copy()
    t[head + nf:head + 2 * nf] = t[head:head + nf]
    clean = np.ones(N, dtype=bool)
    clean[head:head + 2 * nf] = False
    return X, t, theta, s, sigma2, clean


@functools.lru_cache(maxsize=None)
def vecchia_failure_reference(grid):
    """the restatement on its own lists, the clean rows only: dict(nbr, terms, grad, ok, cond)"""
    X, t, theta, s, sigma2, clean = vecchia_failure(grid)
    nbr = vr.ordered_neighbours(X, s, VECCHIA["k"])
    rows = np.flatnonzero(clean)
    terms, g, ok, cond = vr.terms(X, t, s, VECCHIA_FAIL_KERNEL, sigma2, 0., nbr, fit_nugget=False, rows=rows)
    return dict(nbr=nbr, terms=terms, ok=ok, cond=cond, rows=rows)


# ---- C. IterativeGP --------------------------------------------------------------------------------------------------------------------------
ITER_D = 3
N_DOT, N_SEG = DOT_BLOCK + 6, SEG + 4                       # 1030 and 4100
# (n, D, kernel, precond_rank); the restatement's iteration counts are in test_large_design_host.py
ITER_SOLVE_SHAPES = [(N_DOT, ITER_D, "SquaredExponential", 64), (N_DOT, ITER_D, "UniformMat52", 33), (N_SEG, ITER_D, "SquaredExponential", 40),
                     (N_SEG, ITER_D, "Matern52", 256)]
ITER_TAIL = (N_DOT, ITER_D, "SquaredExponential", 64)       # the column that lives in the second block of the dots
ITER_OUTLIER = (N_DOT, ITER_D, "SquaredExponential", 64)    # the argmax across blocks
OUTLIER_ROW, OUTLIER_SHIFT = 1027, 5.
ITER_APPLY = (N_SEG, ITER_D, "SquaredExponential", 40)      # the preconditioner's apply across two segments
APPLY_PROBES = 7
APPLY_FACTOR = 4.                                           # the device's allowance in units of the float64 restatement's own error
ITER_LIK = (N_DOT, ITER_D, 64, "SquaredExponential")        # (n, D, p, kernel), 15 probes
ITER_VAR_SHAPES = [(N_SEG, ITER_D, "SquaredExponential", 40), (N_DOT, ITER_D, "UniformMat52", 33)]
ITER_PREDICT = (N_SEG, ITER_D, "SquaredExponential", 40)


def iter_setup(n, D, kernel, m=dc.M_TEST[0]):
    c = dc.case(n, D, kernel, m=m)
    return c, ir.scales(c.thetas[0][:c.nc], D, kernel)


def tail_column(n, block=DOT_BLOCK):
    """(n, 1): zero on the rows of the first block, nonzero on the rest"""
    b = np.zeros((n, 1))
    b[block:, 0] = np.random.default_rng([5, n]).standard_normal(n - block) + 2.
    return b


def outlier_design(X):
    X = X.copy()
    X[OUTLIER_ROW] += OUTLIER_SHIFT
    return X


def remaining_diagonals(K, L, piv):
    """(rank, N): row t the remaining diagonal before pivot t is chosen, from the columns L of the restatement on the pivots piv"""
    d = np.diag(K)[None, :] - np.vstack([np.zeros((1, L.shape[0])), np.cumsum(L * L, axis=1).T[:-1]])
    for t in range(1, len(piv)):
        d[t, piv[:t]] = 0.
    return d


def apply_probes(n, rank, T=APPLY_PROBES):
    """[(name, g1 (rank, T), g2 (n, T))]: g1 = 0 with g2 zero on the rows of the first segment -- z = sqrt(eta) g2 lives in the second segment
    alone -- and the dense probes of the likelihood tests"""
    g = np.random.default_rng([9, n, T])
    g1, g2 = g.standard_normal((rank, T)), g.standard_normal((n, T))
    tail = g2.copy()
    tail[:SEG] = 0.
    return [("second segment alone", np.zeros((rank, T)), tail), ("dense", g1, g2)]


def _ascending_sums(L, Z, seg=SEG):
    """(L^T L, L^T Z) in float64 with every entry summed over the rows in ascending order, one product and one addition at a time, L^T Z
    segment by segment and the segments in ascending order: the order csrc/kernels_iter.hip documents for gram_kernel and ltv_kernel"""
    p = L.shape[1]
    G, V = np.zeros((p, p)), np.zeros((p, Z.shape[1]))
    for a in range(0, L.shape[0], seg):
        part = np.zeros_like(V)
        for i in range(a, min(a + seg, L.shape[0])):
            G = G + L[i][:, None] * L[i][None, :]
            part = part + L[i][:, None] * Z[i][None, :]
        V = V + part
    return G, V


def apply_restated(L, eta, Z, dtype=np.float64, how="ascending"):
    """P^-1 Z = (Z - L G^-1 L^T Z) / eta, G = eta I + L^T L.  float64, how =
      "ascending"   the sums over the rows in ascending order (_ascending_sums), the explicit symmetrised inverse of
                    iterative_restate.preconditioner, L (G^-1 L^T Z) column by column of L in ascending order: THE float64 restatement
      "factorised"  the same sums, a factorisation of G and two substitutions in place of the inverse
      "blocked"     iterative_restate.preconditioner as it stands: NumPy's blocked sums, which round less than any chain of N additions
    np.longdouble: the factorisation of local_restate, which takes any dtype (the order of its sums is of no account at that precision)"""
    if dtype == np.float64 and how == "blocked":
        pre = ir.preconditioner(L, eta)
        return np.column_stack([pre(np.ascontiguousarray(Z[:, j])) for j in range(Z.shape[1])])
    Ld, Zd = L.astype(dtype), Z.astype(dtype)
    p = L.shape[1]
    if dtype == np.float64:
        G, V = _ascending_sums(Ld, Zd)
        G = G + eta * np.eye(p)
    else:
        G, V = dtype(eta) * np.eye(p, dtype=dtype) + Ld.T @ Ld, Ld.T @ Zd
    if dtype == np.float64 and how == "ascending":
        Ginv = np.linalg.inv(G)
        W2 = (0.5 * (Ginv + Ginv.T)) @ V
    else:
        C = lr.cholesky(G)
        W2 = vr.backward(C, lr.forward(C, V))
    acc = np.zeros_like(Zd)
    for a in range(p):
        acc = acc + Ld[:, a][:, None] * W2[a][None, :]
    return (Zd - acc) / dtype(eta)


def apply_bar(L, eta, Z):
    """(truth in long double (N, T), bar (T,)): per column APPLY_FACTOR times the float64 restatement's own largest distance from the
    long-double evaluation of the same formula on the same L"""
    truth = apply_restated(L, eta, Z, dtype=np.longdouble)
    own = np.max(np.abs(np.asarray(apply_restated(L, eta, Z).astype(np.longdouble) - truth, dtype=np.float64)), axis=0)
    return truth, APPLY_FACTOR * own


def apply_fraction(W, truth, bar):
    return np.max(np.abs(np.asarray(W.astype(np.longdouble) - truth, dtype=np.float64)), axis=0) / bar
