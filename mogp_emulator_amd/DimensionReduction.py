"""
gKDR dimension reduction (Fukumizu and Leng), the counterpart of mogp_emulator/DimensionReduction.py.

The public surface is the reference's: ``gram_matrix``, ``gram_matrix_sqexp`` and ``median_dist`` (host, SciPy, as the
reference computes them), and the class ``gKDR`` with ``K``, ``B``, ``X_scale``, ``Y_scale``, ``__call__`` and
``tune_parameters``.  The matrix R behind B is formed on the device (``libgpgpu.gkdr_R``, csrc/kernels_gkdr.hip); its
M x M eigendecomposition stays on the host with the reference's call and sort.  ``gKDR.grid`` builds every (X_scale,
Y_scale) pair of a tuning grid in one device call, and ``tune_parameters`` makes one such call per fold and reuses
each B for every K it visits.  There is no host fall-back: without the library or a compatible GPU, construction
raises RuntimeError.
"""
import sys

import numpy as np
from scipy.spatial.distance import cdist, pdist, squareform

from . import LibGPGPU

__all__ = ["gKDR", "gram_matrix", "gram_matrix_sqexp", "median_dist"]


def gram_matrix(X, k):
    """The Gram matrix G_ij = k(X_i, X_j) of the rows of X (DimensionReduction.py:68-84)."""
    return cdist(X, X, k)


def gram_matrix_sqexp(X, sigma2):
    """The Gram matrix of X under the squared exponential kernel of variance parameter sigma2 (DimensionReduction.py:86-103)."""
    return np.exp(-0.5 * squareform(pdist(X, 'sqeuclidean')) / sigma2)


def median_dist(X):
    """The median of the pairwise (Euclidean) distances between the rows of X (DimensionReduction.py:106-110)."""
    return np.median(pdist(X))


def k_fold_cross_validation(X, K):
    """(training, validation) partitions of X in its own order (utils.k_fold_cross_validation, randomise=False)."""
    for k in range(K):
        training = [x for i, x in enumerate(X) if i % K != k]
        validation = [x for i, x in enumerate(X) if i % K == k]
        yield training, validation


def device_R(X, Y, sgx2, sgy2, eps, max_pairs_per_pass=0):
    """One device call: (R (nx, ny, M, M), info (nx)) for every pair of squared scales (libgpgpu.gkdr_R).  Every R that
    gKDR uses comes through this function; gKDR.device_calls counts the calls."""
    if not LibGPGPU.HAVE_LIBGPGPU:
        raise RuntimeError("Cannot run gKDR: The GPU library (libgpgpu) could not be loaded")
    if not LibGPGPU.gpu_usable():
        raise RuntimeError("Cannot run gKDR: A compatible GPU could not be found")
    return LibGPGPU.gkdr_R(X, Y, sgx2, sgy2, eps, max_pairs_per_pass)


def _R_grid(X, Y, sgx2, sgy2, eps, max_pairs_per_pass=0):
    gKDR.device_calls += 1
    return device_R(X, Y, sgx2, sgy2, eps, max_pairs_per_pass)


def _not_pd():
    # what scipy.linalg.cho_factor raises for the reference
    return np.linalg.LinAlgError("Kx + N*EPS*I is not positive definite")


class gKDR(object):
    """Dimension reduction by the gKDR method (DimensionReduction.py:113-236).  An instance is callable: it maps inputs
    (N, M) to the reduced coordinates X @ B[:, :K].

    Beyond the reference's attributes (K, B, X_scale, Y_scale) an instance exposes R (the M x M matrix whose eigenvectors
    are B) and eigenvalues (R's eigenvalues in B's order, descending)."""

    #: number of device calls made by this process (tests check that tune_parameters makes one per fold)
    device_calls = 0

    def __init__(self, X, Y, K=None, X_scale=1.0, Y_scale=1.0, EPS=1E-8, SGX=None, SGY=None):
        N, M = np.shape(X)
        if K is None:
            K = M
        assert(K >= 0 and K <= M)
        assert(EPS >= 0)
        assert(SGX is None or SGX > 0.0)
        assert(SGY is None or SGY > 0.0)
        Y = np.reshape(Y, (N, 1))
        if SGX is None:
            SGX = X_scale * median_dist(X)
        if SGY is None:
            SGY = Y_scale * median_dist(Y)
        SGX2 = max(SGX * SGX, sys.float_info.min)
        SGY2 = max(SGY * SGY, sys.float_info.min)
        R, info = _R_grid(np.asarray(X, dtype=np.float64), Y, [SGX2], [SGY2], EPS)
        if info[0]:
            raise _not_pd()
        self._finish(R[0, 0], K, X_scale, Y_scale)

    def _finish(self, R, K, X_scale, Y_scale, keep=None):
        L, V = np.linalg.eigh(R)
        assert(np.allclose(V.imag, 0.0))
        idx = np.argsort(L, 0)[::-1]   # sort descending
        self.X_scale = X_scale
        self.Y_scale = Y_scale
        self.K = K
        if keep is None:
            self.B = V[:, idx]
            self.R = R
        else:
            # a reduction kept by tune_parameters: only the leading `keep` columns of B, no R (M x M each)
            self.B = V[:, idx[:keep]].copy()
        self.eigenvalues = L[idx]

    @classmethod
    def _from_R(cls, R, K, X_scale, Y_scale, keep=None):
        obj = cls.__new__(cls)
        obj._finish(R, K, X_scale, Y_scale, keep)
        return obj

    def _with_K(self, K):
        obj = self.__class__.__new__(self.__class__)
        obj.__dict__.update(self.__dict__)
        obj.K = K
        return obj

    def __call__(self, X):
        """X (N, M) in the unreduced space -> (N, K) in the reduced space."""
        return X @ self.B[:, 0:self.K]

    @classmethod
    def _grid(cls, X, Y, X_scales, Y_scales, K=None, EPS=1E-8, max_pairs_per_pass=0, keep=None):
        """gKDR objects of every (X_scale, Y_scale) pair, row-major, from one device call; None where the matrix of the
        pair's X_scale is not positive definite.  keep: hold only the leading `keep` columns of each B and no R."""
        N, M = np.shape(X)
        if K is None:
            K = M
        assert(K >= 0 and K <= M)
        assert(EPS >= 0)
        X_scales, Y_scales = list(X_scales), list(Y_scales)
        Y = np.reshape(Y, (N, 1))
        mx, my = median_dist(X), median_dist(Y)
        sgx2 = [max((cX * mx) * (cX * mx), sys.float_info.min) for cX in X_scales]
        sgy2 = [max((cY * my) * (cY * my), sys.float_info.min) for cY in Y_scales]
        R, info = _R_grid(np.asarray(X, dtype=np.float64), Y, sgx2, sgy2, EPS, max_pairs_per_pass)
        out = []
        for i, cX in enumerate(X_scales):
            for j, cY in enumerate(Y_scales):
                out.append(None if info[i] else cls._from_R(R[i, j], K, cX, cY, keep))
        return out

    @classmethod
    def grid(cls, X, Y, X_scales, Y_scales, K=None, EPS=1E-8):
        """gKDR(X, Y, K, X_scale, Y_scale, EPS) for every (X_scale, Y_scale) in X_scales x Y_scales, in row-major order,
        from ONE device call.  Raises numpy.linalg.LinAlgError when the matrix of one of the X_scales is not positive
        definite."""
        out = cls._grid(X, Y, X_scales, Y_scales, K, EPS)
        if any(o is None for o in out):
            raise _not_pd()
        return out

    @classmethod
    def tune_parameters(cls, X, Y, train_model, cXs=None, cYs=None,
                        maxK=None, cross_validation_folds=5,
                        verbose=False):
        """(gKDR, loss): the structural dimension K and the scales (cX, cY) that approximately minimise the
        cross-validated L1 loss of `train_model` on the reduced inputs -- the search of DimensionReduction.py:314-433: for
        each (cX, cY), K doubles from 1 until the loss rises or reaches maxK.  The reduction of every (fold, cX, cY) comes
        from one device call per fold over all pairs and serves every K; train_model is called in the reference's order,
        and a pair whose matrix is not positive definite raises numpy.linalg.LinAlgError when the search reaches it."""
        N, M = np.shape(X)
        if cXs is None:
            cXs = [0.5, 1.0, 5.0]
        if cYs is None:
            cYs = [0.5, 1.0, 5.0]
        if maxK is None:
            maxK = M
        assert(maxK >= 1 and maxK <= M)
        cXs, cYs = list(cXs), list(cYs)
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        XY = np.hstack((X, Y[:, np.newaxis]))
        folds = []
        for train, validate in k_fold_cross_validation(XY, cross_validation_folds):
            train = np.array(train)
            validate = np.array(validate)
            # the search uses at most maxK columns of each B; R is not kept (45 M x M matrices at the defaults)
            drs = cls._grid(train[:, 0:-1], train[:, -1], cXs, cYs, keep=maxK)
            folds.append((train, validate, drs))

        def compute_loss(k, cX, cY):
            pair = cXs.index(cX) * len(cYs) + cYs.index(cY)
            err = []
            for train, validate, drs in folds:
                if drs[pair] is None:
                    raise _not_pd()
                dr = drs[pair]._with_K(k)
                model = train_model(dr(train[:, 0:-1]), train[:, -1])
                err.append(np.mean(np.abs(validate[:, -1] - model(dr(validate[:, 0:-1])))))
            return np.mean(err)

        min_loss = np.inf
        argmin_loss = None
        for cX in cXs:
            for cY in cYs:
                loss = np.inf
                params = None
                k = 1
                while (k <= maxK):
                    old_params, params = params, (k, cX, cY)
                    old_loss, loss = loss, compute_loss(*params)

                    if verbose:
                        print("loss(K={}, X_scale={}, Y_scale={}) = {}"
                              .format(*params, loss))

                    if old_loss < loss:
                        if old_loss < min_loss:
                            min_loss = old_loss
                            argmin_loss = old_params
                        break
                    elif k == maxK:
                        if loss < min_loss:
                            min_loss = loss
                            argmin_loss = params
                        break
                    elif 2 * k > maxK:
                        k = maxK
                    else:
                        k *= 2

        dr = gKDR(X, Y, *argmin_loss)
        return (dr, min_loss)
