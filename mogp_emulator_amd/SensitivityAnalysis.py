"""
Variance-based sensitivity analysis of an emulator: first-order and total-effect Sobol indices of its predictive mean, computed on
the device behind the batched prediction (``csrc/kernels_sobol.hip``).

With two independent ``(N, D)`` sample matrices ``A``, ``B`` of the input distribution, ``AB_i`` = ``A`` with column ``i`` taken from
``B``, and ``f`` the predictive mean (mean function included):

    f0   = mean(concat(fA, fB))               V = mean((concat(fA, fB) - f0)**2)
    S_i  = mean((fB - f0) * (fAB_i - fA)) / V           first order (Saltelli 2010)
    ST_i = mean((fA - fAB_i)**2) / (2 V)                total effect (Jansen)

The ``(D + 2) N`` predictions per emulator never leave the device: ``A`` and ``B`` are uploaded once, every ``AB_i`` is built there a
chunk at a time, and ``2 D + 3`` numbers per emulator come back.  Two calls with the same samples return the same bits.
"""
import numpy as np

from .ExperimentalDesign import ExperimentalDesign
from .GaussianProcessGPU import GaussianProcessGPU
from .MultiOutputGP_GPU import MultiOutputGP_GPU


class SobolResult(dict):
    """(first_order, total, mean, variance, emulator_variance) container with dict, attribute and positional access, in the style of
    ``PredictResult``.  ``emulator_variance`` is None unless it was asked for with ``unc=True``."""
    _order = ("first_order", "total", "mean", "variance", "emulator_variance")

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__

    def __getitem__(self, key):
        if isinstance(key, bool) or not isinstance(key, (int, str)):
            raise KeyError(key)
        if isinstance(key, int):
            if not 0 <= key < len(self._order):
                raise KeyError(key)
            key = self._order[key]
        return dict.__getitem__(self, key)

    def __iter__(self):
        return iter([dict.__getitem__(self, k) for k in self._order])

    def __repr__(self):
        if not self.keys():
            return self.__class__.__name__ + "()"
        width = max(len(k) for k in self._order) + 1
        return "\n".join(k.rjust(width) + ": " + repr(self[k]) for k in self._order)


def _samples(D, design, n_base, A, B):
    if (A is None) != (B is None):
        raise ValueError("sobol_indices: pass both A and B, or neither")
    if A is not None:
        if design is not None or n_base is not None:
            raise ValueError("sobol_indices: pass either explicit A, B or a design and n_base, not both")
    else:
        if design is None or n_base is None:
            raise ValueError("sobol_indices: pass either explicit A, B or a design and n_base")
        if not isinstance(design, ExperimentalDesign):
            raise TypeError("sobol_indices: design must be an ExperimentalDesign")
        if design.get_n_parameters() != D:
            raise ValueError("sobol_indices: the design has %d parameters, the emulator %d inputs" % (design.get_n_parameters(), D))
        n_base = int(n_base)
        if n_base < 2:
            raise ValueError("sobol_indices: at least two base samples are needed")
        # in this order: a seeded run reproduces
        A = design.sample(n_base)
        B = design.sample(n_base)
    A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    B = np.ascontiguousarray(np.asarray(B, dtype=np.float64))
    if A.ndim == 1 and D == 1:
        A = A.reshape(-1, 1)
    if B.ndim == 1 and D == 1:
        B = B.reshape(-1, 1)
    if A.ndim != 2 or B.ndim != 2 or A.shape != B.shape:
        raise ValueError("sobol_indices: A and B must be 2D arrays of the same shape")
    if A.shape[1] != D:
        raise ValueError("sobol_indices: the sample matrices must have %d columns, got %d" % (D, A.shape[1]))
    if A.shape[0] < 2:
        raise ValueError("sobol_indices: at least two base samples are needed")
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B))):
        raise ValueError("sobol_indices: the sample matrices must be finite")
    return A, B


def sobol_indices(gp, design=None, n_base=None, A=None, B=None, unc=False, include_nugget=True, allow_not_fit=False):
    """First-order and total-effect Sobol indices of the predictive mean of ``gp``.

    gp: a ``GaussianProcessGPU`` or a ``MultiOutputGP_GPU``, fitted.
    Either explicit sample matrices ``A``, ``B`` of shape ``(N, D)``, or an ``ExperimentalDesign`` and ``n_base``: then
    ``A = design.sample(n_base)`` and ``B = design.sample(n_base)`` are drawn in that order.
    unc: also return ``emulator_variance``, the mean over ``A`` and ``B`` of the predictive variance as ``predict`` reports it
    (``include_nugget`` is passed through) -- the share of the output variance that is code uncertainty, not input uncertainty.
    allow_not_fit (``MultiOutputGP_GPU`` only): emulators that are not fit give NaN rows and do not raise, as in ``predict``.

    Returns a ``SobolResult``: ``first_order``, ``total`` of shape ``(D,)`` and scalar ``mean``, ``variance``, ``emulator_variance``
    for a single GP; ``(n_emulators, D)`` and ``(n_emulators,)`` for a multi-output GP.  A constant emulator (variance 0) has NaN
    indices."""
    if isinstance(gp, GaussianProcessGPU):
        if not gp.theta.data_has_been_set():
            raise ValueError("hyperparameters have not been fit for this Gaussian Process")
        A, B = _samples(gp.D, design, n_base, A, B)
        S, ST, mean, var, ev = gp._densegp_gpu.sobol(A, B, unc=unc, include_nugget=include_nugget)
    elif isinstance(gp, MultiOutputGP_GPU):
        if not allow_not_fit and len(gp.get_indices_not_fit()) > 0:
            raise ValueError("Hyperparameters have not been fit for this Gaussian Process")
        A, B = _samples(gp.D, design, n_base, A, B)
        S, ST, mean, var, ev = gp._mogp_gpu.sobol(A, B, unc=unc, include_nugget=include_nugget)
    else:
        raise TypeError("sobol_indices: gp must be a GaussianProcessGPU or a MultiOutputGP_GPU")
    return SobolResult(first_order=S, total=ST, mean=mean, variance=var, emulator_variance=ev)
