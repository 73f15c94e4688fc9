"""
Validation diagnostics on top of the device path -- the consumers of ``predict(full_cov=True)`` of
mogp_emulator/validation.py:8-482, for ``GaussianProcessGPU`` and ``MultiOutputGP_GPU``:

* ``standard_errors``  (y_pred - y_valid) / sqrt(var), ordered by decreasing predictive variance (validation.py:240-293, 367-398)
* ``pivoted_errors``   L^-1 (y_pred - y_valid)[P] with the pivoted Cholesky factor of the predictive covariance, i.e. the
                       errors de-correlated in order of decreasing conditional variance (validation.py:296-338, 401-441)
* ``mahalanobis``      sum of the squared pivoted errors, optionally scaled by the mean / standard deviation of its
                       Fisher-Snedecor reference distribution (validation.py:8-95); ``generate_mahal_dist`` (validation.py:98-135)

Cross-validation from the training set itself, at the fitted hyperparameters and without refitting (not in the reference):

* ``kfold_labels``     balanced fold labels of n points
* ``cross_validate``   leave-one-out / k-fold held-out predictions, Mahalanobis distances and log scores, computed on the device from the
                       factor of the fit (``Engine::cross_validate``, csrc/kernels_cv.hip); returns a ``CrossValidationResult``

The predictive mean / variance / full covariance come from the batched device prediction and the pivoted factorisation of
each (n_valid x n_valid) covariance from the device routine behind ``nugget="pivot"`` (``LibGPGPU.pivot_cholesky``); what is
left for the host is one triangular solve with n_valid right-hand-side entries.  Same function names, argument meaning,
return shapes and error behaviour as the reference module.
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.stats import f as _fisher_snedecor

from . import LibGPGPU
from .GaussianProcessGPU import GaussianProcessGPU
from .MultiOutputGP_GPU import MultiOutputGP_GPU


class Errors(object):
    "base class of the error definitions (validation.py:341-350)"
    full_cov = False

    def __call__(self, target, mean, cov):
        raise NotImplementedError


class StandardErrors(Errors):
    full_cov = False

    def __call__(self, target, mean, cov):
        P = np.argsort(cov)[::-1]
        return ((mean - target) / np.sqrt(cov))[P], P


class PivotErrors(Errors):
    full_cov = True

    def __call__(self, target, mean, cov):
        # cholesky_factor(cov, 0., "pivot") + ChoInvPivot.solve_L of the reference, factorised on the device
        L, P, _ = LibGPGPU.pivot_cholesky(cov)
        return solve_triangular(L, (mean - target)[P], lower=True), P


def _is_single(gp):
    return isinstance(gp, GaussianProcessGPU)


def _process_inputs(gp, inputs):
    inputs = np.array(inputs, dtype=np.float64)
    if inputs.ndim == 1:
        inputs = inputs.reshape(-1, 1) if gp.D == 1 else inputs.reshape(1, -1)
    return inputs


def _check_valid_data(gp, valid_inputs, valid_targets):
    assert isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)), "Must provide a GP to validate"
    valid_inputs = _process_inputs(gp, valid_inputs)
    valid_targets = np.array(valid_targets)
    if _is_single(gp):
        assert valid_targets.ndim == 1, "Targets for a GP must be a 1D array"
        assert valid_targets.shape[0] == valid_inputs.shape[0], "Bad length for validation targets"
    else:
        assert valid_targets.ndim == 2, "Targets for a MultiOutputGP must be a 2D array"
        assert valid_targets.shape[1] == valid_inputs.shape[0], "Bad shape for validation targets"
    return valid_inputs, valid_targets


def _n_mean(em):
    "number of mean-function coefficients of an emulator, whether they live in theta or are integrated out"
    native = em._densegp_gpu
    return max(int(native.get_theta().get_n_mean()), int(native.get_beta().size))


def compute_errors(gp, valid_inputs, valid_targets, method):
    if isinstance(method, str):
        # (the reference compares the unbound ``method.lower`` and therefore rejects every string, validation.py:210-216;
        # the names it documents are accepted here)
        key = method.lower()
        if key in ("standard", "standarderrors"):
            method = StandardErrors()
        elif key in ("pivot", "pivoterrors"):
            method = PivotErrors()
        else:
            raise ValueError("Bad value for error method in compute_errors")
    assert issubclass(type(method), Errors), "method must be a subclass of Errors"
    valid_inputs, valid_targets = _check_valid_data(gp, valid_inputs, valid_targets)
    mean, cov, _ = gp.predict(valid_inputs, deriv=False, full_cov=method.full_cov)
    if _is_single(gp):
        return method(valid_targets, mean, cov)
    return [method(t, m, c) for t, m, c in zip(valid_targets, mean, cov)]


def standard_errors(gp, valid_inputs, valid_targets):
    return compute_errors(gp, valid_inputs, valid_targets, method=StandardErrors())


def pivoted_errors(gp, valid_inputs, valid_targets):
    return compute_errors(gp, valid_inputs, valid_targets, method=PivotErrors())


def generate_mahal_dist(gp, valid_inputs):
    if _is_single(gp):
        emulators = [gp]
    elif isinstance(gp, MultiOutputGP_GPU):
        emulators = gp.emulators
    else:
        raise TypeError("Provided GP is not a GaussianProcess or MultiOutputGP")
    n_valid = len(_process_inputs(gp, valid_inputs))
    dists = [_fisher_snedecor(dfn=n_valid, dfd=em.n - _n_mean(em) - 2, scale=n_valid) for em in emulators]
    return dists[0] if len(dists) == 1 else dists


def mahalanobis(gp, valid_inputs, valid_targets, scaled=False):
    pivot_errors = pivoted_errors(gp, valid_inputs, valid_targets)
    if _is_single(gp):
        errors = pivot_errors[0]
    else:
        errors = np.array([err[0] for err in pivot_errors])
    M = np.sum(errors ** 2, axis=-1)
    if scaled:
        dists = generate_mahal_dist(gp, valid_inputs)
        single = _is_single(gp) or not isinstance(dists, list)
        M_iter, d_iter = ([M], [dists]) if single else (M, dists)
        out = []
        for M_val, dist in zip(M_iter, d_iter):
            mean, var = dist.stats()
            out.append((M_val - mean) / np.sqrt(var))
        M = np.array(out)
        if _is_single(gp):
            M = M.squeeze(axis=0)
    return M


def kfold_labels(n, k, rng=None):
    """Fold labels of n points for k-fold cross-validation: ``arange(n) % k``, so that the fold sizes differ by at most one; with ``rng``
    (a ``numpy.random.Generator`` or a seed) a permutation of that.  Plain NumPy, the device is not touched."""
    n, k = int(n), int(k)
    if n < 2:
        raise ValueError("kfold_labels: at least two points are needed")
    if k < 2 or k > n:
        raise ValueError("kfold_labels: the number of folds must be between 2 and the number of points")
    labels = np.arange(n) % k
    if rng is not None:
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        labels = rng.permutation(labels)
    return labels


class CrossValidationResult(object):
    """What ``cross_validate`` returns.  For a ``GaussianProcessGPU`` (for a ``MultiOutputGP_GPU`` with a leading emulator axis):

    * ``folds`` (n,)            the fold label of every training point
    * ``mean``, ``unc`` (n,)    held-out predictive mean and variance of every point (variance with or without the nugget, as asked)
    * ``mahalanobis`` (k,)      e_F^T Sigma_F^-1 e_F of every fold, e_F the held-out errors and Sigma_F their predictive covariance
    * ``log_score`` (k,)        log predictive density of the fold's observations given the other folds
    * ``ok`` (k,) bool          False where the fold could not be computed (its entries are NaN)
    * ``standard_errors``       (mean - t) / sqrt(variance with nugget), in training order
    * ``rmse``                  root mean square of the held-out errors
    * ``total_log_score``       sum of ``log_score`` over the folds"""

    def __init__(self, folds, targets, mean, unc, mahalanobis, log_score, ok, nugget, include_nugget):
        self.folds, self.targets, self.mean, self.unc = folds, targets, mean, unc
        self.mahalanobis, self.log_score, self.ok = mahalanobis, log_score, ok
        self.nugget, self.include_nugget = nugget, bool(include_nugget)

    @property
    def k(self):
        return self.mahalanobis.shape[-1]

    @property
    def variance_with_nugget(self):
        if self.include_nugget:
            return self.unc
        return self.unc + np.reshape(self.nugget, np.shape(self.nugget) + (1,) * (self.unc.ndim - np.ndim(self.nugget)))

    @property
    def standard_errors(self):
        return (self.mean - self.targets) / np.sqrt(self.variance_with_nugget)

    @property
    def rmse(self):
        return np.sqrt(np.mean((self.mean - self.targets) ** 2, axis=-1))

    @property
    def total_log_score(self):
        return np.sum(self.log_score, axis=-1)


def cross_validate(gp, k=None, folds=None, rng=None, include_nugget=True, max_slots=0):
    """Leave-one-out or k-fold cross-validation of a fitted ``GaussianProcessGPU`` / ``MultiOutputGP_GPU`` at its fitted hyperparameters:
    every fold is predicted from the other folds without refitting, on the device, from the factor the fit left there.

    ``k=None`` with ``folds=None``: leave-one-out.  ``k``: ``kfold_labels(n, k, rng)``.  ``folds``: the caller's own label vector (n,),
    integers 0 .. k-1 with every label used (``k`` may be omitted or must agree).  ``max_slots`` bounds the (emulator, fold) pairs
    factored per pass (0: the library's choice).  Every argument is checked before the device is touched.  ``RuntimeError`` for
    ``nugget="pivot"``, ``analytic_mean=True`` and a ``GaussianProcessGPU`` that is not fit; emulators of a ``MultiOutputGP_GPU`` that
    are not fit give NaN rows with ``ok`` False.  Returns a ``CrossValidationResult``."""
    if not isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)):
        raise TypeError("cross_validate needs a GaussianProcessGPU or a MultiOutputGP_GPU")
    n = int(gp.n)
    if n < 2:
        raise ValueError("cross_validate: at least two training points are needed")
    if int(max_slots) < 0:
        raise ValueError("cross_validate: max_slots must not be negative")
    if folds is not None:
        labels = np.asarray(folds)
        if labels.ndim != 1 or labels.shape[0] != n:
            raise ValueError("cross_validate: folds must have one label per training point")
        if not np.issubdtype(labels.dtype, np.integer):
            raise ValueError("cross_validate: the fold labels must be integers")
        if labels.min() < 0:
            raise ValueError("cross_validate: the fold labels must not be negative")
        kk = int(labels.max()) + 1 if k is None else int(k)
        if labels.max() >= kk:
            raise ValueError("cross_validate: a fold label is outside [0, k)")
        if kk < 2 or kk > n:
            raise ValueError("cross_validate: the number of folds must be between 2 and the number of training points")
        if np.any(np.bincount(labels, minlength=kk) == 0):
            raise ValueError("cross_validate: every fold needs at least one point")
    elif k is None:
        kk, labels = n, np.arange(n)
    else:
        kk = int(k)
        if kk < 2 or kk > n:
            raise ValueError("cross_validate: the number of folds must be between 2 and the number of training points")
        labels = kfold_labels(n, kk, rng)
    single = _is_single(gp)
    pivot = gp.nugget_type == "pivot" if single else gp._nugget_name == "pivot"
    if pivot:
        raise RuntimeError("cross_validate: not available with nugget=\"pivot\"")
    if getattr(gp, "_analytic_mean", False):
        raise RuntimeError("cross_validate: not available with analytic_mean=True")
    if single:
        native = gp._densegp_gpu
        if not native.theta_fit_status():
            raise RuntimeError("cross_validate: hyperparameters have not been fit for this Gaussian Process")
        targets = np.array(gp.targets, dtype=np.float64)
        mean, var, maha, ls, ok = native.cross_validate(labels, kk, include_nugget=include_nugget, max_slots=max_slots)
        nugget = float(native.get_nugget_size())
    else:
        targets = np.array(gp.targets, dtype=np.float64)
        mean, var, maha, ls, ok = gp._mogp_gpu.cross_validate(labels, kk, include_nugget=include_nugget, max_slots=max_slots)
        nugget = gp._nuggets()
    return CrossValidationResult(folds=np.array(labels), targets=targets, mean=mean, unc=var, mahalanobis=maha, log_score=ls, ok=ok,
                                 nugget=nugget, include_nugget=include_nugget)
