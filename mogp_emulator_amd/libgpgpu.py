"""
``libgpgpu`` -- drop-in replacement for the reference's pybind11 extension of the
same name (mogp_gpu/src/bindings.cu:13-621), backed by the gfx950 C ABI
``libmogp_hip.so`` through ctypes (``_capi``).

``mogp_emulator/LibGPGPU.py:5-14`` does ``from libgpgpu import *``; putting this
module on ``sys.path`` under that name is the whole integration.
The exported names, argument orders, in-place output-buffer conventions and the
``RuntimeError`` behaviour follow the bindings cited next to each definition.

No CPU fallback exists here: import fails if the shared library is missing.
"""
import ctypes

import numpy as np

from . import _capi
from ._capi import check, dptr, iptr

_lib = _capi.load()

__all__ = [
    "have_compatible_device", "fit_GP_MAP", "kernel_type", "nugget_type", "prior_type",
    "BaseMeanFunc", "ZeroMeanFunc", "FixedMeanFunc", "ConstMeanFunc", "PolyMeanFunc",
    "GPParameters", "DenseGP_GPU", "MultiOutputGP_GPU", "GPPriors",
    "WeakPrior", "InvGammaPrior", "GammaPrior", "LogNormalPrior",
    "BaseTransform", "CovTransform", "CorrTransform",
    "SquaredExponentialKernel", "Matern52Kernel", "MeanPriors", "set_fit_options", "set_device", "device_count", "pivot_cholesky",
    "gkdr_R", "design_min_pdist", "design_anneal_lhs", "AnnealResult", "LocalGP_GPU",
]


# --------------------------------------------------------------------------------------
# enums (bindings.cu:585-598; integer values from types.hpp:29-35)
# --------------------------------------------------------------------------------------
class _EnumMeta(type):
    def __iter__(cls):
        return iter(cls._members.values())

    def __call__(cls, value):
        if isinstance(value, cls):
            return value
        try:
            return cls._by_value[int(value)]
        except (KeyError, TypeError, ValueError):
            raise ValueError("%r is not a valid %s" % (value, cls.__name__))


def _make_enum(name, members):
    cls = _EnumMeta(name, (), {"_members": {}, "_by_value": {}})

    def _repr(self):
        return "%s.%s" % (name, self.name)

    cls.__str__ = _repr
    cls.__repr__ = lambda self: "<%s: %d>" % (_repr(self), self.value)
    cls.__int__ = lambda self: self.value
    cls.__index__ = lambda self: self.value
    cls.__eq__ = lambda self, other: isinstance(other, cls) and other.value == self.value
    cls.__ne__ = lambda self, other: not cls.__eq__(self, other)
    cls.__hash__ = lambda self: hash((name, self.value))
    for mname, mval in members:
        obj = object.__new__(cls)
        obj.name, obj.value = mname, mval
        cls._members[mname] = obj
        cls._by_value[mval] = obj
        setattr(cls, mname, obj)
    return cls


# 0, 1: the reference enum (types.hpp:29-35).  2-4: the kernels the reference only has on the CPU (Kernel.py:946-997,
# SURVEY 8f row 4); the uniform kernels share one correlation length over all inputs (n_corr = 1).
kernel_type = _make_enum("kernel_type", [("SquaredExponential", 0), ("Matern52", 1), ("ProductMat52", 2),
                                         ("UniformSqExp", 3), ("UniformMat52", 4)])
# 3: nugget="pivot" of the CPU class (GPParams.py:185-186), not in the reference's GPU enum (types.hpp:29-35)
nugget_type = _make_enum("nugget_type", [("adaptive", 0), ("fit", 1), ("fixed", 2), ("pivot", 3)])
prior_type = _make_enum("prior_type", [("InvGamma", 0), ("Gamma", 1), ("LogNormal", 2), ("Weak", 3)])


def have_compatible_device():
    """bindings.cu:600 / util.hpp:40-47"""
    return bool(_lib.mogp_have_compatible_device())


def device_count():
    return int(_lib.mogp_device_count())


def set_device(i):
    """Select the HIP device for handles created afterwards (one process per GPU)."""
    check(_lib.mogp_set_device(int(i)))


def set_fit_options(max_iter=0, ftol=0., gtol=0., seed=0):
    check(_lib.mogp_set_fit_options(int(max_iter), float(ftol), float(gtol), int(seed)))


def _f64(a, ndim=None, name="array"):
    out = np.ascontiguousarray(a, dtype=np.float64)
    if ndim is not None and out.ndim != ndim:
        raise TypeError("%s must be a %d-D float64 array" % (name, ndim))
    return out


def _outbuf(a, name):
    """Caller-allocated output buffer filled in place (Eigen::Ref semantics, types.hpp:16-18)."""
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"] or not a.flags["WRITEABLE"]:
        raise TypeError("%s must be a writeable C-contiguous float64 ndarray" % name)
    return a


def _cv_labels(labels, n):
    """fold labels of cross_validate as a contiguous int32 vector with one entry per training point"""
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != n:
        raise RuntimeError("cross_validate: one fold label per training point is needed")
    if not np.issubdtype(lab.dtype, np.integer):
        raise RuntimeError("cross_validate: the fold labels must be integers")
    return np.ascontiguousarray(lab, dtype=np.int32)


def _mixture_weight_args(weights, log_q, shape):
    """(weights, log_q) of predict_mixture as contiguous float64 arrays of `shape` or None: exactly one of the two is given"""
    if (weights is None) == (log_q is None):
        raise RuntimeError("predict_mixture: exactly one of weights and log_q must be given")
    out = []
    for a, name in ((weights, "weights"), (log_q, "log_q")):
        if a is not None:
            a = _f64(a, len(shape), name)
            if a.shape != tuple(shape):
                raise RuntimeError("predict_mixture: %s must have shape %s" % (name, tuple(shape)))
        out.append(a)
    return out


def _sample_call(fn, handle, lead, x, n_draws, seed, stream, z, include_nugget, jitter, max_slots, max_draws, return_z):
    """shared by DenseGP_GPU.sample_posterior and MultiOutputGP_GPU.sample_posterior: `lead` = () or (n_emulators,); z None, (S, m) or
    lead + (S, m) -> (samples lead + (S, m), mean lead + (m,), z or None, jitter_used lead, ok lead bool)"""
    m = x.shape[0]
    per = 0
    if z is not None:
        z = _f64(z, name="z")
        if not ((z.ndim == 2 and z.shape[1] == m) or (bool(lead) and z.ndim == 3 and z.shape[0] == lead[0] and z.shape[2] == m)):
            raise ValueError("sample_posterior: z must have shape (n_draws, m)%s" % (" or (n_emulators, n_draws, m)" if lead else ""))
        per = int(z.ndim == 3)
        n_draws = z.shape[-2]
    S = int(n_draws)
    if S < 1:
        raise ValueError("sample_posterior: n_draws must be at least 1")
    samples, mean = np.zeros(lead + (S, m)), np.zeros(lead + (m,))
    zout = np.zeros(lead + (S, m)) if return_z else None
    ju, ok = np.zeros(lead or (1,)), np.zeros(lead or (1,), dtype=np.int32)
    check(fn(handle, dptr(x), m, x.shape[1], S, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, dptr(z), per,
             int(bool(include_nugget)), float(jitter), int(max_slots), int(max_draws), dptr(samples), dptr(mean), dptr(zout), dptr(ju),
             iptr(ok)))
    if not lead:
        return samples, mean, zout, float(ju[0]), bool(ok[0])
    return samples, mean, zout, ju, ok.astype(bool)


def _cov_call(fn, handle, lead, x1, x2, max_slots):
    """shared by DenseGP_GPU.predict_cov and MultiOutputGP_GPU.predict_cov: `lead` = () or (n_emulators,) -> cov lead + (m1, m2)"""
    m1, m2 = x1.shape[0], (x1.shape[0] if x2 is None else x2.shape[0])
    cov = np.zeros(lead + (m1, m2))
    check(fn(handle, dptr(x1), m1, dptr(x2), m2, x1.shape[1], int(max_slots), dptr(cov)))
    return cov


def _alc_call(fn, handle, lead, xc, xr, weights, noise, max_slots, max_points):
    """shared by DenseGP_GPU.alc and MultiOutputGP_GPU.alc: weights (m_r), noise None or lead-or-(1,) -> (reduction lead + (m_c,), cand_var
    lead + (m_c,), ref_var lead + (m_r,), degenerate lead + (m_c,) bool)"""
    mc, mr = xc.shape[0], xr.shape[0]
    w = _f64(weights, 1, "weights")
    if w.shape[0] != mr:
        raise ValueError("alc_criterion: weights must have one entry per reference point")
    if noise is not None:
        noise = _f64(noise, 1, "noise")
        if noise.shape != (lead or (1,)):
            raise ValueError("alc_criterion: noise must have one entry per emulator")
    red, cv, rv = np.zeros(lead + (mc,)), np.zeros(lead + (mc,)), np.zeros(lead + (mr,))
    deg = np.zeros(lead + (mc,), dtype=np.int32)
    check(fn(handle, dptr(xc), mc, dptr(xr), mr, xc.shape[1], dptr(w), dptr(noise), int(max_slots), int(max_points), dptr(red), dptr(cv),
             dptr(rv), iptr(deg)))
    return red, cv, rv, deg.astype(bool)


def _alc_batch_call(fn, handle, lead, x, n_forced, xr, weights, noise, n_points, total, max_slots, keep_scores):
    """shared by DenseGP_GPU.alc_batch and MultiOutputGP_GPU.alc_batch: x (m, D) = the pending points then the candidates, T = n_forced +
    n_points steps -> dict of picks lead + (T,) (-1: none), pick_red lead + (T,), red / deg lead + (T, m) or None, cand_var lead + (m,),
    ref_var / ref_var_after lead + (m_r,), iv lead + (T + 1,), total_picks (T,) or None"""
    m, mr, T = x.shape[0], xr.shape[0], int(n_forced) + int(n_points)
    w = _f64(weights, 1, "weights")
    if w.shape[0] != mr:
        raise ValueError("alc_batch: weights must have one entry per reference point")
    if noise is not None:
        noise = _f64(noise, 1, "noise")
        if noise.shape != (lead or (1,)):
            raise ValueError("alc_batch: noise must have one entry per emulator")
    picks = np.full(lead + (T,), -1, dtype=np.int32)
    pick_red, iv = np.zeros(lead + (T,)), np.zeros(lead + (T + 1,))
    red = np.zeros(lead + (T, m)) if keep_scores else None
    deg = np.zeros(lead + (T, m), dtype=np.int32) if keep_scores else None
    cv, rv, rva = np.zeros(lead + (m,)), np.zeros(lead + (mr,)), np.zeros(lead + (mr,))
    head = (handle, dptr(x), m, int(n_forced), dptr(xr), mr, x.shape[1], dptr(w), dptr(noise), int(n_points))
    tail = (iptr(picks), dptr(pick_red), dptr(red), iptr(deg), dptr(cv), dptr(rv), dptr(rva), dptr(iv))
    tp = None
    if lead:
        tp = np.full(T, -1, dtype=np.int32) if total else None
        check(fn(*(head + (int(bool(total)), int(max_slots)) + tail + (iptr(tp),))))
    else:
        check(fn(*(head + (int(max_slots),) + tail)))
    return dict(picks=picks, pick_red=pick_red, red=red, deg=None if deg is None else deg.astype(bool), cand_var=cv, ref_var=rv,
                ref_var_after=rva, iv=iv, total_picks=tp)


def _sobol_call(fn, handle, D, n_out, A, B, unc, include_nugget):
    """shared by DenseGP_GPU.sobol and MultiOutputGP_GPU.sobol: (S, ST, mean, variance, emulator_variance or None), one row per output"""
    a, b = _f64(A, 2, "A"), _f64(B, 2, "B")
    if a.shape != b.shape:
        raise ValueError("sobol: A and B must have the same shape, got %s and %s" % (a.shape, b.shape))
    if a.shape[1] != D:
        raise ValueError("sobol: the sample matrices must have %d columns, got %d" % (D, a.shape[1]))
    S, ST = np.zeros((n_out, D)), np.zeros((n_out, D))
    mean, var = np.zeros(n_out), np.zeros(n_out)
    ev = np.zeros(n_out) if unc else None
    check(fn(handle, dptr(a), dptr(b), a.shape[0], a.shape[1], int(bool(unc)), int(bool(include_nugget)), dptr(S), dptr(ST),
             dptr(mean), dptr(var), dptr(ev)))
    return S, ST, mean, var, ev


# --------------------------------------------------------------------------------------
# mean functions (bindings.cu:365-413)
# --------------------------------------------------------------------------------------
class BaseMeanFunc(object):
    _h = None

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.mogp_meanfunc_destroy(self._h)
            self._h = None

    def get_n_params(self):
        return int(_lib.mogp_meanfunc_n_params(self._h))

    def _call(self, fn, xs, params, rows):
        xs = _f64(xs)
        if xs.ndim == 1:
            xs = xs.reshape(1, -1)
        p = _f64(np.atleast_1d(params)) if np.size(params) else np.zeros(0)
        m, D = xs.shape
        out = np.zeros(rows(m, D))
        check(fn(self._h, dptr(xs), m, D, dptr(p) if p.size else None, int(p.size), dptr(out)))
        return out

    def mean_f(self, xs, params):
        return self._call(_lib.mogp_meanfunc_mean_f, xs, params, lambda m, D: (m,))

    def mean_deriv(self, xs, params):
        np_ = self.get_n_params()
        if np_ == 0:
            self._call(_lib.mogp_meanfunc_mean_f, xs, params, lambda m, D: (m,))   # length check
            return np.zeros((np.atleast_2d(xs).shape[0], 1))                        # meanfunc.hpp:68-75
        return self._call(_lib.mogp_meanfunc_mean_deriv, xs, params, lambda m, D: (np_, m))

    def mean_inputderiv(self, xs, params):
        return self._call(_lib.mogp_meanfunc_mean_inputderiv, xs, params, lambda m, D: (D, m))


# the native handle never travels: a pickled mean function is rebuilt from its constructor arguments
class ZeroMeanFunc(BaseMeanFunc):
    def __init__(self):
        self._h = _lib.mogp_meanfunc_zero()

    def __reduce__(self):
        return (ZeroMeanFunc, ())


class FixedMeanFunc(BaseMeanFunc):
    def __init__(self, value):
        self._value = float(value)
        self._h = _lib.mogp_meanfunc_fixed(self._value)

    def __reduce__(self):
        return (FixedMeanFunc, (self._value,))


class ConstMeanFunc(BaseMeanFunc):
    def __init__(self):
        self._h = _lib.mogp_meanfunc_const()

    def __reduce__(self):
        return (ConstMeanFunc, ())


class PolyMeanFunc(BaseMeanFunc):
    def __init__(self, dims_powers):
        dp = np.asarray(dims_powers, dtype=np.int32).reshape(-1, 2)
        self._dims = np.ascontiguousarray(dp[:, 0])
        self._pows = np.ascontiguousarray(dp[:, 1])
        self._h = _lib.mogp_meanfunc_poly(iptr(self._dims), iptr(self._pows), int(dp.shape[0]))

    def __reduce__(self):
        return (PolyMeanFunc, (np.stack([self._dims, self._pows], axis=1).tolist(),))


# --------------------------------------------------------------------------------------
# transforms and stand-alone priors (bindings.cu:458-545): host scalar objects
# --------------------------------------------------------------------------------------
class BaseTransform(object):
    pass


class CovTransform(BaseTransform):
    """sigma^2 = exp(theta): gpparams.hpp:72-100"""
    def raw_to_scaled(self, r):
        return np.exp(r)

    def scaled_to_raw(self, s):
        return np.log(s)

    def dscaled_draw(self, s):
        return s

    def d2scaled_draw2(self, s):
        return s


class CorrTransform(BaseTransform):
    """l = exp(-theta/2).  d2scaled_draw2 follows the CPU oracle (+s/4, GPParams.py:69-80); the
    C++ reference has the sign wrong (gpparams.hpp:59-61)."""
    def raw_to_scaled(self, r):
        return np.exp(-0.5 * np.asarray(r))

    def scaled_to_raw(self, s):
        return -2. * np.log(s)

    def dscaled_draw(self, s):
        return -0.5 * np.asarray(s)

    def d2scaled_draw2(self, s):
        return 0.25 * np.asarray(s)


class WeakPrior(object):
    def logp(self, x):
        return 0.

    def dlogpdx(self, x):
        return 0.

    def d2logpdx2(self, x):
        return 0.

    def dlogpdtheta(self, x, transform):
        """chain rule to the raw parameter (gppriors.hpp WeakPrior::dlogpdtheta; Priors.py:617-634)"""
        return float(self.dlogpdx(x) * transform.dscaled_draw(x))

    def d2logpdtheta2(self, x, transform):
        """Priors.py:648-666"""
        return float(self.d2logpdx2(x) * transform.dscaled_draw(x) ** 2 + self.dlogpdx(x) * transform.d2scaled_draw2(x))

    def sample(self, transform=None):
        return float(5. * (np.random.rand() - 0.5))


class _ShapeScalePrior(WeakPrior):
    def __init__(self, shape, scale):
        if not (shape > 0. and scale > 0.):
            raise RuntimeError("shape and scale parameters must be positive")
        self.shape, self.scale = float(shape), float(scale)

    def sample(self, transform=None):
        x = self.sample_x()
        return float(transform.scaled_to_raw(x)) if transform is not None else x


class InvGammaPrior(_ShapeScalePrior):
    def logp(self, x):
        from math import lgamma, log
        return self.shape * log(self.scale) - lgamma(self.shape) - (self.shape + 1.) * log(x) - self.scale / x

    def dlogpdx(self, x):
        return -(self.shape + 1.) / x + self.scale / x ** 2

    def d2logpdx2(self, x):
        return (self.shape + 1.) / x ** 2 - 2. * self.scale / x ** 3

    def sample_x(self):
        return float(self.scale / np.random.gamma(self.shape))


class GammaPrior(_ShapeScalePrior):
    def logp(self, x):
        from math import lgamma, log
        return -self.shape * log(self.scale) - lgamma(self.shape) + (self.shape - 1.) * log(x) - x / self.scale

    def dlogpdx(self, x):
        return (self.shape - 1.) / x - 1. / self.scale

    def d2logpdx2(self, x):
        return -(self.shape - 1.) / x ** 2

    def sample_x(self):
        return float(np.random.gamma(self.shape, self.scale))


class LogNormalPrior(_ShapeScalePrior):
    def logp(self, x):
        from math import log, pi
        return -0.5 * (log(x / self.scale) / self.shape) ** 2 - 0.5 * log(2. * pi) - log(x) - log(self.shape)

    def dlogpdx(self, x):
        from math import log
        return -log(x / self.scale) / self.shape ** 2 / x - 1. / x

    def d2logpdx2(self, x):
        from math import log
        return (-1. / self.shape ** 2 + log(x / self.scale) / self.shape ** 2 + 1.) / x ** 2

    def sample_x(self):
        return float(np.random.lognormal(np.log(self.scale), self.shape))


# --------------------------------------------------------------------------------------
# GPParameters (bindings.cu:415-456 / gpparams.hpp:102-238): host object
# --------------------------------------------------------------------------------------
class GPParameters(object):
    def __init__(self, n_mean=0, n_corr=1, nugget=nugget_type.fit, nugget_size=0.):
        self._n_mean, self._n_corr = int(n_mean), int(n_corr)
        self._nug_type = nugget_type(nugget)
        self._nug_size = float(nugget_size)
        self._has_data = False
        self._mean = np.zeros(self._n_mean)
        self._data = np.zeros(self.get_n_data())

    def get_n_data(self):
        return self._n_corr + 1 + int(self._nug_type == nugget_type.fit)

    def get_n_mean(self):
        return self._n_mean

    def get_n_corr(self):
        return self._n_corr

    def get_data(self):
        return self._data.copy()

    def set_data(self, new):
        new = np.array(new, dtype=np.float64).reshape(-1)
        if new.size != self.get_n_data():
            raise RuntimeError("New data not correct shape")
        self._data = new
        self._has_data = True
        self._mean = np.zeros(self._n_mean)
        if self._nug_type == nugget_type.adaptive:
            self._nug_size = 0.

    def get_mean(self):
        return self._mean.copy()

    def set_mean(self, new):
        self._mean = np.array(new, dtype=np.float64).reshape(-1)
        self._n_mean = self._mean.size

    def get_corr_raw(self):
        return self._data[:self._n_corr].copy()

    def get_corr(self):
        return np.exp(-0.5 * self._data[:self._n_corr])

    def set_corr(self, new):
        self._data[:self._n_corr] = -2. * np.log(np.asarray(new, dtype=np.float64))

    def _cov_index(self):
        return self.get_n_data() - (2 if self._nug_type == nugget_type.fit else 1)

    def get_cov(self):
        return float(np.exp(self._data[self._cov_index()])) if self._has_data else 0.

    def set_cov(self, cov):
        if not self._has_data:
            raise RuntimeError("Need to set data before setting covariance parameter")
        self._data[self._cov_index()] = np.log(cov)

    def get_nugget_type(self):
        return self._nug_type

    def set_nugget_type(self, t):
        self._nug_type = nugget_type(t)

    def get_nugget_size(self):
        if self._nug_type != nugget_type.fit:
            return self._nug_size
        return float(np.exp(self._data[-1]))

    def set_nugget_size(self, size):
        self._nug_size = float(size)
        if self._nug_type == nugget_type.fit and self._data.size:
            self._data[-1] = self._nug_size

    def unset_data(self):
        self._mean = np.zeros(self._n_mean)
        self._data = np.zeros(self.get_n_data())
        self._has_data = False

    def data_has_been_set(self):
        return self._has_data

    def test_same_shape(self, other):
        if isinstance(other, GPParameters):
            return (self._n_mean == other._n_mean and self._n_corr == other._n_corr
                    and self._nug_type == other._nug_type)
        return np.size(other) == self._n_mean + self.get_n_data()


# --------------------------------------------------------------------------------------
# GPPriors proxy (bindings.cu:547-566): the priors live inside the native emulator
# --------------------------------------------------------------------------------------
class GPPriors(object):
    """bindings.cu:528-556 / gppriors.hpp:318-510.  Two forms:

    * ``GPPriors(n_corr, nugget_type)`` -- the constructible container of the native module: ``set_corr`` / ``get_corr`` /
      ``set_cov`` / ``get_cov`` / ``set_nugget`` / ``create_corr_priors`` / ``create_cov_prior`` / ``make_prior`` /
      ``get_logp`` / ``get_dlogpdtheta`` / ``get_d2logpdtheta2`` / ``sample`` on host prior objects (O(D) scalar work;
      arithmetic of the CPU class, Priors.py:291-418);
    * ``GPPriors(emulator)`` (what ``DenseGP_GPU.get_gppriors()`` returns) -- a view on the priors that live inside a
      native emulator; ``get_logp`` / ``get_dlogpdtheta`` / ``sample`` go through the C ABI.
    ``DenseGP_GPU.set_gppriors(priors)`` accepts either."""

    def __init__(self, n_corr_or_owner, nug_type=None):
        if hasattr(n_corr_or_owner, "_h"):
            self._owner = n_corr_or_owner
            return
        self._owner = None
        self._n_corr = int(n_corr_or_owner)
        self._nug_type = nugget_type(nugget_type.fit if nug_type is None else nug_type)
        self._corr = []
        self._cov = None
        self._nug = None
        self._mean = None

    # -- view on a native emulator ---------------------------------------------------------------------------------
    def _data(self, theta):
        return theta.get_data() if isinstance(theta, GPParameters) else _f64(theta)

    # -- container ------------------------------------------------------------------------------------------------------
    def get_nugget_type(self):
        return self._nug_type if self._owner is None else self._owner.get_nugget_type()

    def set_corr(self, newcorr=None):
        """set_corr() appends n_corr weak priors (gppriors.hpp:356-360); set_corr(list) replaces them (:351-354)"""
        self._own_only()
        if newcorr is None:
            self._corr.extend(WeakPrior() for _ in range(self._n_corr))
        else:
            self._corr = list(newcorr)
            self._n_corr = len(self._corr)

    def get_corr(self):
        self._own_only()
        return list(self._corr)

    def set_cov(self, newcov=None):
        self._own_only()
        self._cov = WeakPrior() if newcov is None else newcov

    def get_cov(self):
        self._own_only()
        return self._cov

    def set_nugget(self, new=None):
        """only kept for a fitted nugget (gppriors.hpp:375-391); a (prior_type, [shape, scale]) pair is instantiated"""
        self._own_only()
        if self._nug_type == nugget_type.fit:
            if new is None:
                new = WeakPrior()
            elif isinstance(new, (tuple, list)):
                new = self.make_prior(*new)
            self._nug = new

    def get_nugget(self):
        self._own_only()
        return self._nug

    def get_mean(self):
        self._own_only()
        return self._mean

    def set_mean(self, mean=None):
        self._own_only()
        self._mean = MeanPriors() if mean is None else mean

    @staticmethod
    def make_prior(ptype, priorparams=()):
        """gppriors.hpp:473-488: anything that is not a two-parameter InvGamma / Gamma / LogNormal becomes a weak prior"""
        ptype = prior_type(ptype)
        params = list(priorparams)
        cls = {prior_type.InvGamma: InvGammaPrior, prior_type.Gamma: GammaPrior, prior_type.LogNormal: LogNormalPrior}.get(ptype)
        if cls is not None and len(params) == 2:
            return cls(params[0], params[1])
        return WeakPrior()

    def create_corr_priors(self, all_params):
        """appends one prior per (prior_type, [shape, scale]) pair (gppriors.hpp:490-497)"""
        self._own_only()
        for ptype, params in all_params:
            self._corr.append(self.make_prior(ptype, params))

    def create_cov_prior(self, params):
        self._own_only()
        self._cov = self.make_prior(*params)

    def _own_only(self):
        if self._owner is not None:
            raise RuntimeError("this GPPriors object is a view on an emulator's priors; build a GPPriors(n_corr, nugget_type) to edit")

    def _check_theta(self, theta):
        if not isinstance(theta, GPParameters):
            raise TypeError("theta must be a GPParameters object")
        if not theta.data_has_been_set() or theta.get_n_corr() != len(self._corr) or theta.get_nugget_type() != self._nug_type:
            raise RuntimeError("theta does not match the priors (n_corr, nugget type) or holds no data")
        if self._cov is None or (self._nug_type == nugget_type.fit and self._nug is None):
            raise RuntimeError("covariance / nugget priors have not been set")

    def _terms(self, theta):
        """(prior, scaled value, transform) of every data parameter in theta order"""
        self._check_theta(theta)
        corr = np.atleast_1d(theta.get_corr())
        out = [(pr, float(corr[i]), CorrTransform()) for i, pr in enumerate(self._corr)]
        out.append((self._cov, float(theta.get_cov()), CovTransform()))
        if self._nug_type == nugget_type.fit:
            out.append((self._nug, float(theta.get_nugget_size()), CovTransform()))
        return out

    def get_logp(self, theta):
        if self._owner is not None:
            data = self._data(theta)
            out = np.zeros(1)
            check(_lib.mogp_densegp_priors_logp(self._owner._h, dptr(data), int(data.size), dptr(out)))
            return float(out[0])
        return float(sum(pr.logp(x) for pr, x, _ in self._terms(theta)))

    def get_dlogpdtheta(self, theta):
        if self._owner is not None:
            data = self._data(theta)
            out = np.zeros(data.size)
            check(_lib.mogp_densegp_priors_dlogpdtheta(self._owner._h, dptr(data), int(data.size), dptr(out)))
            return out
        return np.array([pr.dlogpdtheta(x, tr) for pr, x, tr in self._terms(theta)])

    def get_d2logpdtheta2(self, theta):
        """diagonal of the Hessian with respect to the raw parameters (gppriors.hpp:439-456; Priors.py:356-391)"""
        self._own_only()
        return np.array([pr.d2logpdtheta2(x, tr) for pr, x, tr in self._terms(theta)])

    def sample(self):
        if self._owner is not None:
            out = np.zeros(self._owner.n_params() + _lib.mogp_densegp_n_mean(self._owner._h))
            check(_lib.mogp_densegp_priors_sample(self._owner._h, dptr(out)))
            return list(out)
        vals = list(self._mean.sample(CorrTransform())) if self._mean is not None else []      # gppriors.hpp:458-471
        vals += [pr.sample(CorrTransform()) for pr in self._corr]
        vals.append(self._cov.sample(CovTransform()))
        if self._nug_type == nugget_type.fit:
            vals.append(self._nug.sample(CovTransform()))
        return vals

    def native_params(self):
        """(n_corr, corr_params, cov_params, nug_params) for DenseGP_GPU.create_gppriors"""
        self._own_only()

        def spec(pr):
            for t, cls in ((prior_type.InvGamma, InvGammaPrior), (prior_type.Gamma, GammaPrior), (prior_type.LogNormal, LogNormalPrior)):
                if isinstance(pr, cls):
                    return (t, [pr.shape, pr.scale])
            return (prior_type.Weak, [0., 0.])
        return len(self._corr), [spec(pr) for pr in self._corr], spec(self._cov), spec(self._nug)


def _prior_spec(spec):
    t, p = spec
    p = list(p) + [0., 0.]
    return int(prior_type(t)), float(p[0]), float(p[1])


def _pack_priors(n_corr, corr_params, cov_params, nug_params):
    ct = np.zeros(max(n_corr, 1), dtype=np.int32)
    cp = np.zeros(2 * max(n_corr, 1))
    if len(corr_params) != n_corr:
        raise RuntimeError("number of correlation priors must equal n_corr")
    for d, spec in enumerate(corr_params):
        ct[d], cp[2 * d], cp[2 * d + 1] = _prior_spec(spec)
    cvt, a, b = _prior_spec(cov_params)
    cov = np.array([a, b])
    ngt, a, b = _prior_spec(nug_params)
    nug = np.array([a, b])
    return ct, cp, cvt, cov, ngt, nug


# --------------------------------------------------------------------------------------
# DenseGP_GPU (bindings.cu:14-257)
# --------------------------------------------------------------------------------------
class DenseGP_GPU(object):
    def __init__(self, inputs, targets, testing_size, meanfunc=None, kern=kernel_type.SquaredExponential,
                 nugtype=nugget_type.adaptive, nugsize=0., _borrowed=None, _parent=None, analytic_mean=False):
        if _borrowed is not None:
            self._h, self._owns, self._parent = _borrowed, False, _parent
            self._meanfunc = meanfunc
            return
        X = _f64(inputs, 2, "inputs")
        t = _f64(targets, 1, "targets")
        if t.shape[0] != X.shape[0]:
            raise RuntimeError("inputs and targets must have the same first dimension")
        if meanfunc is None:
            meanfunc = ZeroMeanFunc()
        self._meanfunc = meanfunc
        create = _lib.mogp_densegp_create_analytic_mean if analytic_mean else _lib.mogp_densegp_create
        self._h = create(dptr(X), X.shape[0], X.shape[1], dptr(t), int(testing_size), meanfunc._h,
                         int(kernel_type(kern)), int(nugget_type(nugtype)), float(nugsize))
        if not self._h:
            raise RuntimeError(_capi.last_error())
        self._owns, self._parent = True, None

    def __del__(self):
        if getattr(self, "_owns", False) and getattr(self, "_h", None):
            _lib.mogp_densegp_destroy(self._h)
            self._h = None

    # -- shape / data -------------------------------------------------------------------
    def n(self):
        return int(_lib.mogp_densegp_n(self._h))

    def D(self):
        return int(_lib.mogp_densegp_D(self._h))

    def n_corr(self):
        return int(_lib.mogp_densegp_n_corr(self._h))

    def n_params(self):
        return int(_lib.mogp_densegp_n_params(self._h))

    def inputs(self):
        out = np.zeros((self.n(), self.D()))
        check(_lib.mogp_densegp_inputs(self._h, dptr(out)))
        return out

    def targets(self):
        out = np.zeros(self.n())
        check(_lib.mogp_densegp_targets(self._h, dptr(out)))
        return out

    def set_mean_priors(self, q, b, Binv, Binv_b, logdetB):
        """MeanPriors of the analytic mean: b (q), B^-1 (q, q), B^-1 b (q), log|B|; q = 0 -> weak"""
        b, Binv, Binv_b = _f64(b, 1, "b"), np.ascontiguousarray(Binv, dtype=np.float64), _f64(Binv_b, 1, "Binv_b")
        check(_lib.mogp_densegp_set_mean_priors(self._h, int(q), dptr(b), dptr(Binv), dptr(Binv_b), float(logdetB)))

    def get_beta(self):
        """analytically fitted mean coefficients (analytic_mean=True only; theta.mean of the CPU class)"""
        nb = int(_lib.mogp_densegp_n_beta(self._h))
        out = np.zeros(max(nb, 1))
        check(_lib.mogp_densegp_get_beta(self._h, dptr(out)))
        return out[:nb].copy()

    # -- parameters -----------------------------------------------------------------------
    def theta_fit_status(self):
        return bool(_lib.mogp_densegp_theta_fit_status(self._h))

    def reset_theta_fit_status(self):
        check(_lib.mogp_densegp_reset_theta_fit_status(self._h))

    def get_theta(self):
        nm, nd = _lib.mogp_densegp_n_mean(self._h), _lib.mogp_densegp_n_data(self._h)
        p = GPParameters(nm, self.n_corr(), self.get_nugget_type(), 0.)
        data, mean = np.zeros(nd), np.zeros(max(nm, 1))
        check(_lib.mogp_densegp_get_theta(self._h, dptr(data), dptr(mean)))
        p._data, p._mean = data, mean[:nm].copy()
        p._has_data = self.theta_fit_status()
        p._nug_size = self.get_nugget_size()
        return p

    def get_gppriors(self):
        return GPPriors(self)

    def set_gppriors(self, priors):
        """bindings.cu:62-65: attach a GPPriors(n_corr, nugget_type) container (its distributions are copied into the
        native emulator; mean priors go through set_mean_priors)"""
        if not isinstance(priors, GPPriors) or priors._owner is not None:
            raise RuntimeError("set_gppriors: expected a GPPriors(n_corr, nugget_type) container")
        n_corr, corr, cov, nug = priors.native_params()
        if priors.get_cov() is None:
            raise RuntimeError("set_gppriors: the covariance prior has not been set")
        self.create_gppriors(n_corr, corr, cov, nug)

    def create_gppriors(self, n_corr, corr_params, cov_params, nug_params):
        ct, cp, cvt, cov, ngt, nug = _pack_priors(int(n_corr), corr_params, cov_params, nug_params)
        check(_lib.mogp_densegp_create_gppriors(self._h, int(n_corr), iptr(ct), dptr(cp), cvt, dptr(cov), ngt, dptr(nug)))

    def get_nugget_size(self):
        return float(_lib.mogp_densegp_get_nugget_size(self._h))

    def set_nugget_size(self, v):
        check(_lib.mogp_densegp_set_nugget_size(self._h, float(v)))

    def get_nugget_type(self):
        return nugget_type(_lib.mogp_densegp_get_nugget_type(self._h))

    def set_nugget_type(self, t):
        check(_lib.mogp_densegp_set_nugget_type(self._h, int(nugget_type(t))))

    def get_kernel_type(self):
        return kernel_type(_lib.mogp_densegp_get_kernel_type(self._h))

    def get_kernel(self):
        return _KERNEL_OBJECTS[int(self.get_kernel_type())]()

    def get_meanfunc(self):
        return self._meanfunc

    # -- fit / objective --------------------------------------------------------------------
    @staticmethod
    def _theta_vec(theta):
        if isinstance(theta, GPParameters):
            return np.concatenate([theta.get_mean(), theta.get_data()])
        return _f64(np.atleast_1d(theta), 1, "theta")

    def fit(self, theta):
        th = self._theta_vec(theta)
        check(_lib.mogp_densegp_fit(self._h, dptr(th), int(th.size)))

    def get_logpost(self, theta):
        th = self._theta_vec(theta)
        out = np.zeros(1)
        check(_lib.mogp_densegp_get_logpost(self._h, dptr(th), int(th.size), dptr(out)))
        return float(out[0])

    def logpost_deriv(self, result):
        _outbuf(result, "result")
        check(_lib.mogp_densegp_logpost_deriv(self._h, dptr(result), int(result.size)))

    def logpost_hessian(self, theta):
        """Hessian of the negative log-posterior at theta, (n_params, n_params), computed on the device (both triangles, exactly
        symmetric).  A fitted emulator keeps its cached state.  RuntimeError for nugget "pivot", the analytic mean, a mean function
        with parameters in theta, ProductMat52, and a theta at which the covariance matrix cannot be factorised."""
        th = self._theta_vec(theta)
        out = np.zeros((th.size, th.size))
        check(_lib.mogp_densegp_logpost_hessian(self._h, dptr(th), int(th.size), dptr(out)))
        return out

    def predict_mixture(self, thetas, testing, weights=None, log_q=None, include_nugget=True, max_slots=0, max_points=0):
        """Prediction averaged over the S hyperparameter samples thetas (S, n_params), reduced over the samples on the device:
        (mean, within, between (m,), weights, logpost (S,), ok (S,) bool).  Exactly one of weights (S,) and log_q (S,); the fitted
        state of the emulator is not touched.  See mogp_densegp_predict_mixture (include/mogp_hip.h)."""
        th = _f64(thetas, 2, "thetas")
        x = self._testing(testing)
        S, m = th.shape[0], x.shape[0]
        w, q = _mixture_weight_args(weights, log_q, (S,))
        mean, within, between = np.zeros(m), np.zeros(m), np.zeros(m)
        wout, lp, ok = np.zeros(S), np.zeros(S), np.zeros(S, dtype=np.int32)
        check(_lib.mogp_densegp_predict_mixture(self._h, dptr(th), S, th.shape[1], dptr(w), dptr(q), dptr(x), m, x.shape[1],
                                                int(bool(include_nugget)), int(max_slots), int(max_points), dptr(mean), dptr(within),
                                                dptr(between), dptr(wout), dptr(lp), iptr(ok)))
        return mean, within, between, wout, lp, ok.astype(bool)

    def cross_validate(self, labels, k, include_nugget=True, max_slots=0):
        """Leave-one-out / k-fold predictive errors at the fitted hyperparameters, on the device and without refitting: labels (n,)
        ints in [0, k) -> (mean, var (n,), mahalanobis, log_score (k,), ok (k,) bool).  The fitted state of the emulator is not
        touched.  See mogp_densegp_cross_validate (include/mogp_hip.h)."""
        n = self.n()
        lab = _cv_labels(labels, n)
        k = int(k)
        mean, var = np.zeros(n), np.zeros(n)
        maha, ls, ok = np.zeros(max(k, 0)), np.zeros(max(k, 0)), np.zeros(max(k, 0), dtype=np.int32)
        check(_lib.mogp_densegp_cross_validate(self._h, iptr(lab), n, k, int(bool(include_nugget)), int(max_slots), dptr(mean), dptr(var),
                                               dptr(maha), dptr(ls), iptr(ok)))
        return mean, var, maha, ls, ok.astype(bool)

    def sample_posterior(self, testing, n_draws=1, seed=0, stream=0, z=None, include_nugget=True, jitter=0., max_slots=0, max_draws=0,
                         return_z=False):
        """n_draws joint draws of the emulated function at testing (m, D), factored and multiplied on the device:
        (samples (S, m), mean (m,), z (S, m) or None, jitter_used, ok).  z (S, m): the caller's normals, else generated on the device from
        (seed, stream).  The fitted state of the emulator is not touched.  See mogp_densegp_sample_posterior (include/mogp_hip.h)."""
        return _sample_call(_lib.mogp_densegp_sample_posterior, self._h, (), self._testing(testing), n_draws, seed, stream, z,
                            include_nugget, jitter, max_slots, max_draws, return_z)

    def predict_cov(self, x1, x2=None, max_slots=0):
        """Posterior covariance (m1, m2) of the latent function between the points x1 (m1, D) and x2 (m2, D; None: x1), nugget not
        included.  See mogp_densegp_predict_cov (include/mogp_hip.h)."""
        return _cov_call(_lib.mogp_densegp_predict_cov, self._h, (), self._testing(x1), None if x2 is None else self._testing(x2), max_slots)

    def alc(self, candidates, reference, weights, noise=None, max_slots=0, max_points=0):
        """The ALC criterion of the candidates (m_c, D) over the reference points (m_r, D) with weights (m_r): (reduction (m_c,), cand_var
        (m_c,), ref_var (m_r,), degenerate (m_c,) bool); noise: a float or None (the nugget of the fit).  See mogp_densegp_alc."""
        return _alc_call(_lib.mogp_densegp_alc, self._h, (), self._testing(candidates), self._testing(reference), weights,
                         None if noise is None else np.array([float(noise)]), max_slots, max_points)

    def alc_batch(self, x, n_forced, reference, weights, n_points, noise=None, max_slots=0, keep_scores=True):
        """A greedy ALC batch on the device, the posterior conditioned on every pick: x (m, D) = n_forced pending points, then the
        candidates.  See _alc_batch_call for what comes back and mogp_densegp_alc_batch (include/mogp_hip.h) for the rules."""
        return _alc_batch_call(_lib.mogp_densegp_alc_batch, self._h, (), self._testing(x), n_forced, self._testing(reference), weights,
                               None if noise is None else np.array([float(noise)]), n_points, False, max_slots, keep_scores)

    # -- predict ------------------------------------------------------------------------------
    def _testing(self, testing):
        x = _f64(testing)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        if x.ndim != 2:
            raise TypeError("testing must be a 2-D array")
        return x

    def predict(self, testing):
        x = _f64(testing).reshape(-1)
        out = np.zeros(1)
        check(_lib.mogp_densegp_predict(self._h, dptr(x), int(x.size), dptr(out)))
        return float(out[0])

    def predict_variance(self, testing, var):
        x = _f64(testing).reshape(-1)
        _outbuf(var, "var")
        mean, v = np.zeros(1), np.zeros(1)
        check(_lib.mogp_densegp_predict_variance(self._h, dptr(x), int(x.size), dptr(mean), dptr(v)))
        var.reshape(-1)[0] = v[0]
        return float(mean[0])

    def predict_batch(self, testing, result):
        x = self._testing(testing)
        _outbuf(result, "result")
        check(_lib.mogp_densegp_predict_batch(self._h, dptr(x), x.shape[0], x.shape[1], dptr(result), int(result.size)))

    def predict_variance_batch(self, testing, mean, var):
        x = self._testing(testing)
        _outbuf(mean, "mean")
        _outbuf(var, "var")
        check(_lib.mogp_densegp_predict_variance_batch(self._h, dptr(x), x.shape[0], x.shape[1], dptr(mean), dptr(var),
                                                       int(min(mean.size, var.size))))

    def predict_deriv(self, testing, result):
        x = self._testing(testing)
        _outbuf(result, "result")
        if result.ndim != 2:
            raise RuntimeError("predict_deriv: the result buffer passed was the wrong shape to hold the result")
        check(_lib.mogp_densegp_predict_deriv(self._h, dptr(x), x.shape[0], x.shape[1], dptr(result), result.shape[0],
                                              result.shape[1]))

    def predict_full_cov(self, testing, mean, cov):
        """mean (m,), cov (m, m): full predictive covariance WITHOUT nugget (GaussianProcess.py:899-911)"""
        x = self._testing(testing)
        _outbuf(mean, "mean")
        _outbuf(cov, "cov")
        if mean.size < x.shape[0] or cov.size < x.shape[0] ** 2:
            raise RuntimeError("predict_full_cov: The result buffer passed was too small to hold the covariance")
        check(_lib.mogp_densegp_predict_full_cov(self._h, dptr(x), x.shape[0], x.shape[1], dptr(mean), dptr(cov)))

    def implausibility(self, testing, obs, obs_var=0., discrepancy=0., include_nugget=True):
        """|obs - E f(x)| / sqrt(Var f(x) [+ nugget] + discrepancy + obs_var) for every row of testing, computed on
        the device behind the prediction (HistoryMatching.py:262-276)."""
        x = self._testing(testing)
        out = np.zeros(x.shape[0])
        check(_lib.mogp_densegp_implausibility(self._h, dptr(x), x.shape[0], x.shape[1], float(obs), float(obs_var),
                                               float(discrepancy), int(bool(include_nugget)), dptr(out)))
        return out

    def sobol(self, A, B, unc=False, include_nugget=True):
        """first-order and total-effect Sobol indices of the predictive mean from the sample matrices A, B (N, D), computed on the
        device behind the prediction: (S (D,), ST (D,), mean, variance, emulator_variance or None)"""
        S, ST, mean, var, ev = _sobol_call(_lib.mogp_densegp_sobol, self._h, self.D(), 1, A, B, unc, include_nugget)
        return S[0], ST[0], float(mean[0]), float(var[0]), (float(ev[0]) if unc else None)

    def loo_variance(self):
        """leave-one-out predictive variance 1/[K^-1]_ii at every training input (MICEFastGP.fast_predict for all indices)"""
        out = np.zeros(self.n())
        check(_lib.mogp_densegp_loo_variance(self._h, dptr(out)))
        return out

    # -- matrices -------------------------------------------------------------------------------
    def _fill_nn(self, fn, out, name):
        _outbuf(out, name)
        if out.size < self.n() * self.n():
            raise RuntimeError("%s: the buffer passed is too small" % name)
        check(fn(self._h, dptr(out)))

    def get_K(self, K_h):
        self._fill_nn(_lib.mogp_densegp_get_K, K_h, "get_K")

    def get_invQ(self, invQ_h):
        self._fill_nn(_lib.mogp_densegp_get_invQ, invQ_h, "get_invQ")

    def get_cholesky_lower(self, result):
        self._fill_nn(_lib.mogp_densegp_get_cholesky_lower, result, "get_cholesky_lower")

    def get_pivot(self):
        """(P, rank) of the current fit: K[P][:, P] = L L^T (ChoInvPivot.P, linalg/cholesky.py:82-104); the identity and
        n unless the nugget type is ``pivot``."""
        P = np.zeros(self.n(), dtype=np.int32)
        rank = ctypes.c_int(0)
        check(_lib.mogp_densegp_get_pivot(self._h, iptr(P), ctypes.byref(rank)))
        return P, rank.value

    def get_invQt(self, invQt_h):
        _outbuf(invQt_h, "invQt_h")
        if invQt_h.size < self.n():
            raise RuntimeError("get_invQt: the buffer passed is too small")
        check(_lib.mogp_densegp_get_invQt(self._h, dptr(invQt_h)))


# --------------------------------------------------------------------------------------
# MultiOutputGP_GPU (bindings.cu:260-337)
# --------------------------------------------------------------------------------------
class MultiOutputGP_GPU(object):
    def __init__(self, inputs, targets, testing_size, meanfunc=None, kern=kernel_type.SquaredExponential,
                 nugtype=nugget_type.adaptive, nugsize=0., analytic_mean=False, devices=None):
        """devices: None -- one engine on the current device; a list of ordinals -- the emulators split into contiguous blocks,
        one engine per non-empty block on devices[k] (mogp_mogp_create_on_devices; a device may be repeated)"""
        X = _f64(inputs, 2, "inputs")
        T = np.ascontiguousarray(np.array([np.asarray(t, dtype=np.float64) for t in targets]))
        if T.ndim != 2 or T.shape[1] != X.shape[0]:
            raise RuntimeError("targets must have shape (n_emulators, n)")
        if meanfunc is None:
            meanfunc = ZeroMeanFunc()
        self._meanfunc = meanfunc
        if devices is None:
            create = _lib.mogp_mogp_create_analytic_mean if analytic_mean else _lib.mogp_mogp_create
            self._h = create(dptr(X), X.shape[0], X.shape[1], dptr(T), T.shape[0], int(testing_size), meanfunc._h,
                             int(kernel_type(kern)), int(nugget_type(nugtype)), float(nugsize))
        else:
            dev = np.ascontiguousarray(np.asarray(list(devices), dtype=np.int32).reshape(-1))
            self._h = _lib.mogp_mogp_create_on_devices(dptr(X), X.shape[0], X.shape[1], dptr(T), T.shape[0], int(testing_size),
                                                       meanfunc._h, int(kernel_type(kern)), int(nugget_type(nugtype)), float(nugsize),
                                                       int(bool(analytic_mean)), iptr(dev), int(dev.size))
        if not self._h:
            raise RuntimeError(_capi.last_error())

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.mogp_mogp_destroy(self._h)
            self._h = None

    def n(self):
        return int(_lib.mogp_mogp_n(self._h))

    def D(self):
        return int(_lib.mogp_mogp_D(self._h))

    def n_emulators(self):
        return int(_lib.mogp_mogp_n_emulators(self._h))

    def n_parts(self):
        return int(_lib.mogp_mogp_n_parts(self._h))

    def parts(self):
        """[(device, lo, hi)] of every part: the engine on `device` holds emulators [lo, hi)"""
        out = []
        for k in range(self.n_parts()):
            d, lo, hi = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
            check(_lib.mogp_mogp_part(self._h, k, ctypes.byref(d), ctypes.byref(lo), ctypes.byref(hi)))
            out.append((d.value, lo.value, hi.value))
        return out

    def inputs(self):
        out = np.zeros((self.n(), self.D()))
        check(_lib.mogp_mogp_inputs(self._h, dptr(out)))
        return out

    def targets(self):
        out = np.zeros((self.n_emulators(), self.n()))
        check(_lib.mogp_mogp_targets(self._h, dptr(out)))
        return [row.copy() for row in out]

    def targets_at_index(self, index):
        return self.targets()[index]

    def emulator(self, index):
        h = _lib.mogp_mogp_emulator(self._h, int(index))
        if not h:
            raise RuntimeError(_capi.last_error())
        return DenseGP_GPU(None, None, 0, meanfunc=self._meanfunc, _borrowed=h, _parent=self)

    def n_data_params(self):
        return [self.emulator(i).n_params() for i in range(self.n_emulators())]

    def n_corr_params(self):
        return [self.emulator(0).n_corr()] * self.n_emulators()

    def get_nugget_type(self):
        return nugget_type(_lib.mogp_mogp_get_nugget_type(self._h))

    def get_nugget_size(self):
        return float(_lib.mogp_mogp_get_nugget_size(self._h))

    def _indices(self, fn):
        out = np.zeros(self.n_emulators(), dtype=np.int32)
        c = fn(self._h, iptr(out))
        return [int(i) for i in out[:c]]

    def get_fitted_indices(self):
        return self._indices(_lib.mogp_mogp_get_fitted_indices)

    def get_unfitted_indices(self):
        return self._indices(_lib.mogp_mogp_get_unfitted_indices)

    def reset_fit_status(self):
        check(_lib.mogp_mogp_reset_fit_status(self._h))

    def create_priors_for_emulator(self, emulator_index, n_corr, corr_params, cov_params, nug_params):
        ct, cp, cvt, cov, ngt, nug = _pack_priors(int(n_corr), corr_params, cov_params, nug_params)
        check(_lib.mogp_mogp_create_priors_for_emulator(self._h, int(emulator_index), int(n_corr), iptr(ct), dptr(cp), cvt,
                                                        dptr(cov), ngt, dptr(nug)))

    def fit_emulator(self, index, theta):
        th = DenseGP_GPU._theta_vec(theta)
        check(_lib.mogp_mogp_fit_emulator(self._h, int(index), dptr(th), int(th.size)))

    def fit(self, thetas):
        if len(thetas) and isinstance(thetas[0], GPParameters):
            thetas = [DenseGP_GPU._theta_vec(t) for t in thetas]
        th = _f64(thetas, 2, "thetas")
        check(_lib.mogp_mogp_fit(self._h, dptr(th), th.shape[0], th.shape[1]))

    def eval(self, thetas, grad=True):
        """Batched objective (+ gradient) of every emulator at its own theta: ONE device pass.
        Returns (logpost (n_out,), grad (n_out, n_params) or None, ok (n_out,) bool)."""
        th = _f64(thetas, 2, "thetas")
        f = np.zeros(th.shape[0])
        g = np.zeros(th.shape) if grad else None
        ok = np.zeros(th.shape[0], dtype=np.int32)
        check(_lib.mogp_mogp_eval(self._h, dptr(th), th.shape[0], th.shape[1], dptr(f), dptr(g), iptr(ok)))
        return f, g, ok.astype(bool)

    def hessian(self, thetas):
        """Hessians of every emulator at its own row of thetas (n_emulators, widest n_params) in ONE batched device call per part:
        (hess (n_emulators, P, P), ok (n_emulators,) bool).  A row that starts with NaN is skipped; its block, and that of a
        row at which the factorisation fails, is NaN with ok False.  An emulator with fewer parameters than the widest fills the
        leading block of its own size; the rest of its block is NaN."""
        th = _f64(thetas, 2, "thetas")
        hess = np.zeros((th.shape[0], th.shape[1], th.shape[1]))
        ok = np.zeros(th.shape[0], dtype=np.int32)
        check(_lib.mogp_mogp_hessian(self._h, dptr(th), th.shape[0], th.shape[1], dptr(hess), iptr(ok)))
        return hess, ok.astype(bool)

    def _testing(self, testing):
        x = _f64(testing)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        return x

    def predict(self, testing):
        x = self._testing(testing)[:1]
        out = np.zeros((self.n_emulators(), 1))
        check(_lib.mogp_mogp_predict_batch(self._h, dptr(x), 1, x.shape[1], dptr(out)))
        return out[:, 0]

    def predict_batch(self, testing, results):
        x = self._testing(testing)
        _outbuf(results, "results")
        if results.size < self.n_emulators() * x.shape[0]:
            raise RuntimeError("predict_batch: the result buffer passed was too small to hold the result")
        check(_lib.mogp_mogp_predict_batch(self._h, dptr(x), x.shape[0], x.shape[1], dptr(results)))

    def predict_variance_batch(self, testing, means, vars):
        x = self._testing(testing)
        _outbuf(means, "means")
        _outbuf(vars, "vars")
        if min(means.size, vars.size) < self.n_emulators() * x.shape[0]:
            raise RuntimeError("predict_variance_batch: The result buffer passed was too small to hold the variance")
        check(_lib.mogp_mogp_predict_variance_batch(self._h, dptr(x), x.shape[0], x.shape[1], dptr(means), dptr(vars)))

    def predict_deriv(self, testing, results):
        x = self._testing(testing)
        if isinstance(results, (list, tuple)):
            buf = np.zeros((self.n_emulators(), x.shape[0], x.shape[1]))
            check(_lib.mogp_mogp_predict_deriv(self._h, dptr(x), x.shape[0], x.shape[1], dptr(buf)))
            for r, b in zip(results, buf):
                r[...] = b
            return
        _outbuf(results, "results")
        if results.size < self.n_emulators() * x.size:
            raise RuntimeError("predict_deriv: the result buffer passed was the wrong shape to hold the result")
        check(_lib.mogp_mogp_predict_deriv(self._h, dptr(x), x.shape[0], x.shape[1], dptr(results)))

    def predict_full_cov(self, testing, means, covs):
        """means (n_out, m), covs (n_out, m, m) for every fitted emulator, one batched device pass (no nugget)"""
        x = self._testing(testing)
        _outbuf(means, "means")
        _outbuf(covs, "covs")
        if means.size < self.n_emulators() * x.shape[0] or covs.size < self.n_emulators() * x.shape[0] ** 2:
            raise RuntimeError("predict_full_cov: The result buffer passed was too small to hold the covariance")
        check(_lib.mogp_mogp_predict_full_cov(self._h, dptr(x), x.shape[0], x.shape[1], dptr(means), dptr(covs)))

    def implausibility(self, testing, obs, obs_var, discrepancy, include_nugget=True, rank=1):
        """history-matching score of every row of testing over all outputs, one number per point (device-fused)"""
        x = self._testing(testing)
        ne = self.n_emulators()
        z = np.ascontiguousarray(np.broadcast_to(np.asarray(obs, dtype=np.float64), (ne,)))
        ov = np.ascontiguousarray(np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (ne,)))
        dc = np.ascontiguousarray(np.broadcast_to(np.asarray(discrepancy, dtype=np.float64), (ne,)))
        out = np.zeros(x.shape[0])
        check(_lib.mogp_mogp_implausibility(self._h, dptr(x), x.shape[0], x.shape[1], dptr(z), dptr(ov), dptr(dc),
                                            int(bool(include_nugget)), int(rank), dptr(out)))
        return out

    def sobol(self, A, B, unc=False, include_nugget=True):
        """Sobol indices of every emulator in one batched pass per part: (S, ST (n_emulators, D), mean, variance, emulator_variance
        or None (n_emulators,)); rows of emulators that are not fit are NaN"""
        return _sobol_call(_lib.mogp_mogp_sobol, self._h, self.D(), self.n_emulators(), A, B, unc, include_nugget)

    def predict_mixture(self, thetas, testing, weights=None, log_q=None, include_nugget=True, max_slots=0, max_points=0):
        """DenseGP_GPU.predict_mixture for every emulator, all (emulator, sample) pairs of a part in one batched pass: thetas
        (n_emulators, S, widest n_params), weights or log_q (n_emulators, S) -> (mean, within, between (n_emulators, m), weights,
        logpost (n_emulators, S), ok (n_emulators, S) bool, ok_all (n_emulators,) bool).  Rows of emulators that are not fit are NaN."""
        th = _f64(thetas, 3, "thetas")
        x = self._testing(testing)
        ne = self.n_emulators()
        if th.shape[0] != ne:
            raise RuntimeError("thetas must have one block of samples per emulator")
        S, m = th.shape[1], x.shape[0]
        w, q = _mixture_weight_args(weights, log_q, (ne, S))
        mean, within, between = np.zeros((ne, m)), np.zeros((ne, m)), np.zeros((ne, m))
        wout, lp, ok = np.zeros((ne, S)), np.zeros((ne, S)), np.zeros((ne, S), dtype=np.int32)
        ok_all = np.zeros(ne, dtype=np.int32)
        check(_lib.mogp_mogp_predict_mixture(self._h, dptr(th), S, th.shape[2], dptr(w), dptr(q), dptr(x), m, x.shape[1],
                                             int(bool(include_nugget)), int(max_slots), int(max_points), dptr(mean), dptr(within),
                                             dptr(between), dptr(wout), dptr(lp), iptr(ok), iptr(ok_all)))
        return mean, within, between, wout, lp, ok.astype(bool), ok_all.astype(bool)

    def cross_validate(self, labels, k, include_nugget=True, max_slots=0):
        """DenseGP_GPU.cross_validate for every emulator with the same folds, all (emulator, fold) pairs of a part in batched
        passes: (mean, var (n_emulators, n), mahalanobis, log_score (n_emulators, k), ok (n_emulators, k) bool).  Rows of emulators
        that are not fit are NaN with ok False."""
        n, ne = self.n(), self.n_emulators()
        lab = _cv_labels(labels, n)
        k = int(k)
        kk = max(k, 0)
        mean, var = np.zeros((ne, n)), np.zeros((ne, n))
        maha, ls, ok = np.zeros((ne, kk)), np.zeros((ne, kk)), np.zeros((ne, kk), dtype=np.int32)
        check(_lib.mogp_mogp_cross_validate(self._h, iptr(lab), n, k, int(bool(include_nugget)), int(max_slots), dptr(mean), dptr(var),
                                            dptr(maha), dptr(ls), iptr(ok)))
        return mean, var, maha, ls, ok.astype(bool)

    def sample_posterior(self, testing, n_draws=1, seed=0, stream=0, z=None, include_nugget=True, jitter=0., max_slots=0, max_draws=0,
                         return_z=False):
        """DenseGP_GPU.sample_posterior for every emulator, max_slots emulators per pass: (samples (n_emulators, S, m), mean
        (n_emulators, m), z or None, jitter_used (n_emulators,), ok (n_emulators,) bool); emulator e draws from stream + e.  z: (S, m)
        shared or (n_emulators, S, m).  Rows of emulators that are not fit are NaN with ok False."""
        return _sample_call(_lib.mogp_mogp_sample_posterior, self._h, (self.n_emulators(),), self._testing(testing), n_draws, seed, stream,
                            z, include_nugget, jitter, max_slots, max_draws, return_z)

    def predict_cov(self, x1, x2=None, max_slots=0):
        """DenseGP_GPU.predict_cov for every emulator: (n_emulators, m1, m2); rows of emulators that are not fit are NaN."""
        return _cov_call(_lib.mogp_mogp_predict_cov, self._h, (self.n_emulators(),), self._testing(x1),
                         None if x2 is None else self._testing(x2), max_slots)

    def alc(self, candidates, reference, weights, noise=None, max_slots=0, max_points=0):
        """DenseGP_GPU.alc for every emulator, max_slots emulators per group and max_points reference points per chunk: (reduction, cand_var
        (n_emulators, m_c), ref_var (n_emulators, m_r), degenerate (n_emulators, m_c) bool); noise (n_emulators,) or None.  Rows of
        emulators that are not fit are NaN."""
        return _alc_call(_lib.mogp_mogp_alc, self._h, (self.n_emulators(),), self._testing(candidates), self._testing(reference), weights,
                         noise, max_slots, max_points)

    def alc_batch(self, x, n_forced, reference, weights, n_points, noise=None, total=False, max_slots=0, keep_scores=True):
        """DenseGP_GPU.alc_batch for every emulator (total False) or one batch for the model (total True: total_picks (T,)); noise
        (n_emulators,) or None.  Rows of emulators that are not fit are NaN with picks of -1.  See mogp_mogp_alc_batch."""
        return _alc_batch_call(_lib.mogp_mogp_alc_batch, self._h, (self.n_emulators(),), self._testing(x), n_forced,
                               self._testing(reference), weights, noise, n_points, total, max_slots, keep_scores)

    def predict_variance_batch_dev(self, d_testing, m, d_means, d_vars):
        """Device-pointer variant: inputs already resident in HBM, results stay in HBM."""
        check(_lib.mogp_mogp_predict_variance_batch_dev(self._h, int(d_testing), int(m), self.D(), int(d_means), int(d_vars)))

    def predict_dev(self, d_testing, m, d_means, d_vars=None, d_derivs=None):
        """Device pointers throughout: means (+ variances, + input derivatives (n_emulators, m, D)) of every emulator in one pass,
        results stay in HBM; any mean function; rows of emulators that are not fit are NaN."""
        check(_lib.mogp_mogp_predict_dev(self._h, int(d_testing), int(m), self.D(), int(d_means),
                                         int(d_vars) if d_vars else None, int(d_derivs) if d_derivs else None))


def fit_GP_MAP(gp, n_tries=15, theta0=()):
    """bindings.cu:602-605 / fitting.hpp:61-128"""
    th = _f64(np.atleast_1d(np.asarray(theta0, dtype=np.float64))) if np.size(theta0) else np.zeros(0)
    ptr = dptr(th) if th.size else None
    if isinstance(gp, DenseGP_GPU):
        check(_lib.mogp_fit_single_GP_MAP(gp._h, int(n_tries), ptr, int(th.size)))
    elif isinstance(gp, MultiOutputGP_GPU):
        check(_lib.mogp_fit_GP_MAP(gp._h, int(n_tries), ptr, int(th.size)))
    else:
        raise TypeError("fit_GP_MAP(): incompatible function arguments")
    return gp


def pivot_cholesky(A):
    """(L, P, rank) = pivoted Cholesky of a symmetric matrix with positive diagonal, computed on the device with the
    semantics of linalg/cholesky.py:284-327 (LAPACK dpstrf; skipped rows get the decreasing replacement diagonal)."""
    A = _f64(np.asarray(A, dtype=np.float64))
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("A must have shape (n,n)")
    n = A.shape[0]
    L = np.zeros((n, n))
    P = np.zeros(n, dtype=np.int32)
    rank = ctypes.c_int(0)
    check(_lib.mogp_pivot_cholesky(dptr(A), n, dptr(L), iptr(P), ctypes.byref(rank)))
    return L, P, rank.value


def gkdr_R(X, y, sgx2, sgy2, eps, max_pairs_per_pass=0):
    """(R, info) of gKDR (DimensionReduction.py:132-236) for every pair of squared kernel scales, in one device call:
    R (len(sgx2), len(sgy2), M, M), info (len(sgx2)) non-zero where Kx + N eps I is not positive definite (those R are NaN)."""
    X = _f64(X, 2, "X")
    n, m = X.shape
    y = _f64(np.reshape(y, (-1,)), 1, "y")
    if y.shape[0] != n:
        raise ValueError("y must have one entry per row of X")
    sx = _f64(np.atleast_1d(sgx2), 1, "sgx2")
    sy = _f64(np.atleast_1d(sgy2), 1, "sgy2")
    R = np.empty((sx.size, sy.size, m, m))
    info = np.zeros(sx.size, dtype=np.int32)
    check(_lib.mogp_gkdr_R(dptr(X), n, m, dptr(y), sx.size, dptr(sx), sy.size, dptr(sy), float(eps), int(max_pairs_per_pass),
                           dptr(R), iptr(info)))
    return R, info


def design_min_pdist(designs):
    """Smallest pairwise Euclidean distance of every design of ``designs`` (T, n, D) -- ``pdist(d).min()`` of
    ExperimentalDesign.py:665 for all tries of a maximin search in one device call; returns an array (T,).  A single design (n, D)
    counts as T = 1.  n = 1 has no pair: ValueError, as ``np.min`` of the empty ``pdist`` raises."""
    designs = _f64(designs)
    if designs.ndim == 2:
        designs = designs[None]
    if designs.ndim != 3:
        raise TypeError("designs must be a (T, n, D) float64 array")
    T, n, D = designs.shape
    if n < 2:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    if not np.all(np.isfinite(designs)):
        raise ValueError("designs must be finite")
    out = np.empty(T)
    if T:
        check(_lib.mogp_design_min_pdist(dptr(designs), T, n, D, dptr(out)))
    return out


class AnnealResult(object):
    """What ``design_anneal_lhs`` returns, one entry per chain: ``levels`` (C, n, D) int32 the best level matrix, ``phi`` (C) its criterion,
    ``min_r`` (C) its smallest integer squared distance, ``pairs`` (C) the pairs at that minimum, ``accepted`` (C) the accepted proposals.
    ``winner``: the chain with the largest ``min_r``, then the fewest ``pairs``, then the lowest index -- all exact integers."""

    def __init__(self, levels, phi, min_r, pairs, accepted):
        self.levels, self.phi, self.min_r, self.pairs, self.accepted = levels, phi, min_r, pairs, accepted

    @property
    def winner(self):
        return min(range(len(self.min_r)), key=lambda c: (-int(self.min_r[c]), int(self.pairs[c]), c))


def design_anneal_lhs(start, n_steps, q=5, theta0=0.1, rho=0.9, stage=None, seed=0, stream=0):
    """Column-swap threshold accepting on Morris & Mitchell's criterion from every level matrix of ``start`` (C, n, D) (one matrix (n, D)
    counts as C = 1; every column a permutation of 0 .. n-1), ``n_steps`` proposals per chain, on the device (csrc/kernels_lhs.hip; the
    algorithm: DESIGN.md section 3 "Design").  ``stage`` (None: max(1, n_steps // 100)) proposals share one threshold, which starts at
    ``theta0`` and is multiplied by ``rho`` after each stage.  Chain c uses the Philox stream ``stream + c`` under ``seed``.  Returns an
    ``AnnealResult``.  The library refuses by name what it cannot serve (RuntimeError)."""
    raw = np.asarray(start)
    if raw.dtype.kind not in "iu":
        raise TypeError("start must be an integer array of levels")
    if raw.ndim == 2:
        raw = raw[None]
    if raw.ndim != 3 or raw.size == 0:
        raise TypeError("start must be a non-empty (C, n, D) integer array")
    C, n, D = raw.shape
    if raw.min() < 0 or raw.max() >= n:
        raise RuntimeError("design_anneal_lhs: the levels of start must lie in 0 .. n-1")
    levels = np.ascontiguousarray(raw, dtype=np.int32)
    n_steps = int(n_steps)
    stage = max(1, n_steps // 100) if stage is None else int(stage)
    best = np.empty((C, n, D), dtype=np.int32)
    phi = np.empty(C)
    min_r, pairs, accepted = (np.empty(C, dtype=np.int64) for _ in range(3))
    ll = ctypes.POINTER(ctypes.c_longlong)
    check(_lib.mogp_design_anneal_lhs(iptr(levels), C, n, D, n_steps, int(q), float(theta0), float(rho), stage,
                                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, iptr(best), dptr(phi),
                                      min_r.ctypes.data_as(ll), pairs.ctypes.data_as(ll), accepted.ctypes.data_as(ll)))
    return AnnealResult(best, phi, min_r, pairs, accepted)


class LocalGP_GPU(object):
    """Native handle of ``LocalGP`` (csrc/kernels_local.hip): the design ``inputs`` (N, D) and the residual targets ``residuals`` (E, N) stay
    on ``device`` (None: the current device) until ``close()``.  The arguments are taken as they are: ``LocalGP.py`` has checked them."""

    def __init__(self, inputs, residuals, device=None):
        self._h = None
        inputs, residuals = _f64(inputs, 2, "inputs"), _f64(residuals, 2, "residuals")
        self.N, self.D = inputs.shape
        self.E = residuals.shape[0]
        h = _lib.mogp_local_create(dptr(inputs), self.N, self.D, dptr(residuals), self.E, -1 if device is None else int(device))
        if not h:
            raise RuntimeError(_capi.last_error())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _lib.mogp_local_destroy(self._h)
            self._h = None

    __del__ = close

    def predict(self, emulator, kern, scale, sigma2, nugget, jitter, include_nugget, testing, k, max_points=0, unc=True,
                return_neighbours=False):
        """(mean (m), unc (m) or None, ok (m) bool, radius (m), neighbours (m, k) int64 or None) of row ``emulator`` of the residuals"""
        if not self._h:
            raise RuntimeError("predict_local: the handle has been closed")
        testing, scale = _f64(testing, 2, "testing"), _f64(scale, 1, "scale")
        m = testing.shape[0]
        mean, radius, ok = np.empty(m), np.empty(m), np.empty(m, dtype=np.int32)
        var = np.empty(m) if unc else None
        nbr = np.empty((m, int(k)), dtype=np.int32) if return_neighbours else None
        check(_lib.mogp_local_predict(self._h, int(emulator), int(kern), dptr(scale), float(sigma2), float(nugget), float(jitter),
                                      int(bool(include_nugget)), dptr(testing), m, testing.shape[1], int(k), int(max_points), dptr(mean),
                                      dptr(var), iptr(ok), dptr(radius), iptr(nbr)))
        return mean, var, ok.astype(bool), radius, None if nbr is None else nbr.astype(np.int64)

    def vecchia_neighbours(self, scale, k, return_neighbours=True):
        """The ordered search (row t sees rows < t) in the metric ``scale``; the lists stay on the device.  (N, k) int64 in the handle's own
        numbering, -1 behind the min(t, k) neighbours of row t, or None"""
        if not self._h:
            raise RuntimeError("vecchia_neighbours: the handle has been closed")
        scale = _f64(scale, 1, "scale")
        nbr = np.empty((self.N, int(k)), dtype=np.int32) if return_neighbours else None
        check(_lib.mogp_local_vecchia_neighbours(self._h, dptr(scale), int(k), iptr(nbr)))
        return None if nbr is None else nbr.astype(np.int64)

    def vecchia_loglik(self, emulator, kern, scale, sigma2, nugget, jitter, k, grad=False, return_terms=False, max_points=0):
        """(value, grad (D + 2) or None, terms (N) or None, ok (N) bool) of row ``emulator`` of the residuals on the lists of the last search"""
        if not self._h:
            raise RuntimeError("vecchia_loglik: the handle has been closed")
        scale = _f64(scale, 1, "scale")
        value, ok = np.empty(1), np.empty(self.N, dtype=np.int32)
        g = np.empty(self.D + 2) if grad else None
        terms = np.empty(self.N) if return_terms else None
        check(_lib.mogp_local_vecchia_loglik(self._h, int(emulator), int(kern), dptr(scale), float(sigma2), float(nugget), float(jitter), int(k),
                                             int(bool(grad)), int(max_points), dptr(value), dptr(g), dptr(terms), iptr(ok)))
        return float(value[0]), g, terms, ok.astype(bool)

    # ---- iterative exact prediction (csrc/engine_iter.hip, csrc/kernels_iter.hip) ----
    def kmatvec(self, kern, scale, sigma2, nugget, V, queries=None):
        """(sigma2 k(X, X) + nugget I) V, or sigma2 k(queries, X) V with ``queries`` (m, D); V (N, r)"""
        if not self._h:
            raise RuntimeError("kmatvec: the handle has been closed")
        scale, V = _f64(scale, 1, "scale"), _f64(V, 2, "V")
        q = None if queries is None else _f64(queries, 2, "queries")
        out = np.empty((self.N if q is None else q.shape[0], V.shape[1]))
        check(_lib.mogp_local_kmatvec(self._h, int(kern), dptr(scale), float(sigma2), float(nugget), dptr(q), 0 if q is None else q.shape[0],
                                      self.D if q is None else q.shape[1], dptr(V), V.shape[1], dptr(out)))
        return out

    def precondition(self, kern, scale, sigma2, nugget, rank, return_factor=False):
        """Builds and keeps the preconditioner; (rank reached, pivots (rank reached) int64 or None, L (N, rank reached) or None)"""
        if not self._h:
            raise RuntimeError("precondition: the handle has been closed")
        scale, rank = _f64(scale, 1, "scale"), int(rank)
        got = np.zeros(1, dtype=np.int32)
        piv = np.zeros(max(rank, 1), dtype=np.int32) if return_factor else None
        L = np.zeros((self.N, max(rank, 1))) if return_factor else None
        check(_lib.mogp_local_precondition(self._h, int(kern), dptr(scale), float(sigma2), float(nugget), rank, iptr(got), iptr(piv), dptr(L)))
        r = int(got[0])
        if not return_factor:
            return r, None, None
        return r, piv[:r].astype(np.int64), np.ascontiguousarray(L[:, :r])

    def solve(self, B, rtol, max_iter):
        """(x (N, c), iterations (c) int64, converged (c) bool, residual (c)) at the hyperparameters of the last ``precondition``"""
        if not self._h:
            raise RuntimeError("solve: the handle has been closed")
        B = _f64(B, 2, "B")
        c = B.shape[1]
        x, res = np.empty_like(B), np.empty(c)
        it, cv = np.empty(c, dtype=np.int32), np.empty(c, dtype=np.int32)
        check(_lib.mogp_local_solve(self._h, dptr(B), c, float(rtol), int(max_iter), dptr(x), iptr(it), iptr(cv), dptr(res)))
        return x, it.astype(np.int64), cv.astype(bool), res

    def predict_exact(self, emulator, kern, scale, sigma2, nugget, rank, rtol, max_iter, include_nugget, testing, unc=False, max_points=0,
                      return_alpha=False):
        """(mean (m), unc (m) or None, (iterations, converged, residual) of the alpha solve, (iterations (m), converged (m), residual (m)) of the
        variance solves or None, alpha (N) or None); ``testing`` None: alpha alone"""
        if not self._h:
            raise RuntimeError("predict_exact: the handle has been closed")
        scale = _f64(scale, 1, "scale")
        t = None if testing is None else _f64(testing, 2, "testing")
        m = 0 if t is None else t.shape[0]
        want = bool(unc) and m > 0
        mean = np.empty(m) if m else None
        var, vres = (np.empty(m), np.empty(m)) if want else (None, None)
        vst = np.empty((m, 2), dtype=np.int32) if want else None
        st, res = np.empty(2, dtype=np.int32), np.empty(1)
        alpha = np.empty(self.N) if return_alpha else None
        check(_lib.mogp_local_predict_exact(self._h, int(emulator), int(kern), dptr(scale), float(sigma2), float(nugget), int(rank), float(rtol),
                                            int(max_iter), int(bool(include_nugget)), dptr(t), m, self.D if t is None else t.shape[1],
                                            int(max_points), dptr(mean), dptr(var), iptr(st), dptr(res), iptr(vst), dptr(vres), dptr(alpha)))
        vstats = (vst[:, 0].astype(np.int64), vst[:, 1].astype(bool), vres) if want else None
        return mean, var, (int(st[0]), bool(st[1]), float(res[0])), vstats, alpha

    def variance_bound(self, kern, scale, sigma2, nugget, rank, include_nugget, testing, var_rank=0, max_points=0, return_cache=False):
        """(bound (m) or None, the columns of the cache that entered, R (N, rank of the cache) or None) of ``mogp_local_variance_bound``;
        ``testing`` None: the cache alone.  ``var_rank`` 0: every column of the cache"""
        if not self._h:
            raise RuntimeError("variance_bound: the handle has been closed")
        scale, rank = _f64(scale, 1, "scale"), int(rank)
        t = None if testing is None else _f64(testing, 2, "testing")
        m = 0 if t is None else t.shape[0]
        var = np.empty(m) if m else None
        got = np.zeros(1, dtype=np.int32)
        R = np.zeros((self.N, max(rank, 1))) if return_cache else None
        check(_lib.mogp_local_variance_bound(self._h, int(kern), dptr(scale), float(sigma2), float(nugget), rank, int(var_rank),
                                             int(bool(include_nugget)), dptr(t), m, self.D if t is None else t.shape[1], int(max_points), dptr(var),
                                             iptr(got), dptr(R)))
        r = int(got[0])
        return var, r, None if R is None else np.ascontiguousarray(R[:, :r])

    # ---- pathwise posterior draws (csrc/engine_rff.hip, csrc/kernels_rff.hip) ----
    def rff(self, scale, omega, phase, W, amp, queries=None, max_points=0):
        """(S, M) amp sum_f W[s][f] cos(phase[f] + omega[f] . (x * scale)) at the design's rows, or at ``queries`` (m, D); omega (F, D), W (S, F)"""
        if not self._h:
            raise RuntimeError("rff: the handle has been closed")
        scale, omega, phase, W = _f64(scale, 1, "scale"), _f64(omega, 2, "omega"), _f64(phase, 1, "phase"), _f64(W, 2, "W")
        q = None if queries is None else _f64(queries, 2, "queries")
        out = np.empty((W.shape[0], self.N if q is None else q.shape[0]))
        check(_lib.mogp_local_rff(self._h, dptr(scale), dptr(q), 0 if q is None else q.shape[0], omega.shape[1], dptr(omega), dptr(phase),
                                  omega.shape[0], dptr(W), W.shape[0], float(amp), int(max_points), dptr(out)))
        return out

    # ---- input derivatives at large designs (csrc/kernels_iter.hip kinderiv_kernel, csrc/kernels_rff.hip rff_inderiv_kernel) ----
    def kmatvec_inputderiv(self, kern, scale, sigma2, V, queries, max_points=0):
        """(m, D, r) d/dx_d [sigma2 k(queries, X) V] with respect to the raw coordinates of ``queries`` (m, D); V (N, r)"""
        if not self._h:
            raise RuntimeError("kmatvec_inputderiv: the handle has been closed")
        scale, V, q = _f64(scale, 1, "scale"), _f64(V, 2, "V"), _f64(queries, 2, "queries")
        if V.shape[0] != self.N:
            raise RuntimeError("kmatvec_inputderiv: V must have N rows")
        out = np.empty((q.shape[0], q.shape[1], V.shape[1]))
        check(_lib.mogp_local_kmatvec_inputderiv(self._h, int(kern), dptr(scale), float(sigma2), dptr(q), q.shape[0], q.shape[1], dptr(V),
                                                 V.shape[1], int(max_points), dptr(out)))
        return out

    def rff_inputderiv(self, scale, omega, phase, W, amp, queries, max_points=0):
        """(S, m, D) the derivative of ``rff`` with respect to the raw coordinates of ``queries`` (m, D)"""
        if not self._h:
            raise RuntimeError("rff_inputderiv: the handle has been closed")
        scale, omega, phase, W = _f64(scale, 1, "scale"), _f64(omega, 2, "omega"), _f64(phase, 1, "phase"), _f64(W, 2, "W")
        q = _f64(queries, 2, "queries")
        if q.shape[1] != omega.shape[1] or W.shape[1] != omega.shape[0] or phase.shape[0] != omega.shape[0]:
            raise RuntimeError("rff_inputderiv: queries (m, D), omega (F, D), phase (F,) and W (S, F) do not fit together")
        out = np.empty((W.shape[0], q.shape[0], q.shape[1]))
        check(_lib.mogp_local_rff_inputderiv(self._h, dptr(scale), dptr(q), q.shape[0], omega.shape[1], dptr(omega), dptr(phase), omega.shape[0],
                                             dptr(W), W.shape[0], float(amp), int(max_points), dptr(out)))
        return out

    def sample_paths(self, emulator, kern, scale, sigma2, nugget, rank, rtol, max_iter, omega, phase, n_draws, amp, seed, stream, first_draw,
                     feature_normals=None, noise_normals=None):
        """(W (S, F) the weights' normals used, v (S, N), iterations (S) int64, converged (S) bool, residual (S), the rank the preconditioner
        reached) of ``mogp_local_sample_paths``"""
        if not self._h:
            raise RuntimeError("sample_paths: the handle has been closed")
        scale, omega, phase = _f64(scale, 1, "scale"), _f64(omega, 2, "omega"), _f64(phase, 1, "phase")
        Win = None if feature_normals is None else _f64(feature_normals, 2, "feature_normals")
        Ein = None if noise_normals is None else _f64(noise_normals, 2, "noise_normals")
        S, F = int(n_draws), omega.shape[0]
        W, v, res = np.empty((S, F)), np.empty((S, self.N)), np.empty(S)
        st, got = np.empty((S, 2), dtype=np.int32), np.zeros(1, dtype=np.int32)
        check(_lib.mogp_local_sample_paths(self._h, int(emulator), int(kern), dptr(scale), float(sigma2), float(nugget), int(rank), float(rtol),
                                           int(max_iter), dptr(omega), dptr(phase), F, S, float(amp), int(seed), int(stream), int(first_draw),
                                           dptr(Win), dptr(Ein), dptr(W), dptr(v), iptr(st), dptr(res), iptr(got)))
        return W, v, st[:, 0].astype(np.int64), st[:, 1].astype(bool), res, int(got[0])

    def loglik_exact(self, emulator, kern, scale, sigma2, nugget, rank, rtol, max_iter, g1, g2, grad=False, probe_terms=False,
                     return_panels=False):
        """The pieces of the exact log-likelihood (``mogp_local_loglik_exact``) as a dict: ``y_alpha``, ``alpha_alpha``, ``logdet_g``,
        ``rank``, per column (the data column first) ``iterations``, ``converged``, ``residual``, per probe ``rho`` and ``uw``, ``coef``
        (max_iter, 2, 1 + T), ``forms_data`` / ``forms_probe`` (D,) with ``grad``, ``forms_each`` (T, D) with ``probe_terms``, and ``z`` (N, T),
        ``x`` = [alpha | u_t] and ``w`` = [alpha | w_t] (N, 1 + T) with ``return_panels``.  g1 (rank reached, T), g2 (N, T)."""
        if not self._h:
            raise RuntimeError("loglik_exact: the handle has been closed")
        scale, g1, g2 = _f64(scale, 1, "scale"), _f64(g1, 2, "g1"), _f64(g2, 2, "g2")
        T, C, D = g2.shape[1], g2.shape[1] + 1, self.D
        sc, st, res = np.zeros(4), np.zeros((C, 2), dtype=np.int32), np.zeros(C)
        rho, uw, coef = np.zeros(T), np.zeros(T), np.zeros((int(max_iter), 2, C))
        forms = np.zeros(2 * D) if grad else None
        each = np.zeros((T, D)) if grad and probe_terms else None
        z, x, w = (np.zeros((self.N, T)), np.zeros((self.N, C)), np.zeros((self.N, C))) if return_panels else (None, None, None)
        check(_lib.mogp_local_loglik_exact(self._h, int(emulator), int(kern), dptr(scale), float(sigma2), float(nugget), int(rank), float(rtol),
                                           int(max_iter), dptr(g1) if g1.size else None, g1.shape[0], dptr(g2), T, int(bool(grad)), dptr(sc),
                                           iptr(st), dptr(res), dptr(rho), dptr(uw), dptr(coef), dptr(forms), dptr(each), dptr(z), dptr(x), dptr(w)))
        return dict(y_alpha=float(sc[0]), alpha_alpha=float(sc[1]), logdet_g=float(sc[2]), rank=int(sc[3]), iterations=st[:, 0].astype(np.int64),
                    converged=st[:, 1].astype(bool), residual=res, rho=rho, uw=uw, coef=coef, forms_data=None if forms is None else forms[:D],
                    forms_probe=None if forms is None else forms[D:], forms_each=each, z=z, x=x, w=w)


# --------------------------------------------------------------------------------------
# stand-alone kernel objects (bindings.cu:340-361; flat layouts of kernel.hpp:47-107), evaluated on the
# device (mogp_kernel_eval): there is no host implementation of the covariance in the product.
# params = [corr_raw (n_corr), log sigma^2], as the native objects of the reference take them.
# --------------------------------------------------------------------------------------
class _KernelBase(object):
    _kt = kernel_type.SquaredExponential

    def get_n_params(self, inputs):
        return int(np.atleast_2d(inputs).shape[1])

    def _eval(self, what, x1, x2, params):
        x1, x2 = np.atleast_2d(_f64(x1)), np.atleast_2d(_f64(x2))
        if x1.shape[1] != x2.shape[1]:
            raise RuntimeError("kernel inputs must have the same number of columns")
        p = _f64(params, 1)
        n1, D = x1.shape
        n2 = x2.shape[0]
        nc = self.get_n_params(x1)
        out = np.zeros({0: n1 * n2, 1: (nc + 1) * n1 * n2, 2: n2 * n1 * D}[what])
        check(_lib.mogp_kernel_eval(int(self._kt), what, dptr(x1), n1, dptr(x2), n2, D, dptr(p), int(p.size), dptr(out)))
        return out, (n1, n2, D, nc)

    def kernel_f(self, x1, x2, params):
        """sigma^2 k(x1_i, x2_j), shape (n1, n2)"""
        out, (n1, n2, _, _) = self._eval(0, x1, x2, params)
        return out.reshape(n1, n2)

    def kernel_deriv(self, x1, x2, params):
        """d/d theta_p of kernel_f as a flat array of n_params * n1 * n2 entries in (p, i, j) order (the reference returns
        it flat, kernel.hpp:89-107; ``.reshape(n_params, n1, n2)`` is the CPU class's array, Kernel.py:133-173)"""
        return self._eval(1, x1, x2, params)[0]

    def kernel_inputderiv(self, x1, x2, params):
        """d/d x1_i[d] of kernel_f as a flat array of n1 * n2 * D entries in (j, i, d) order (kernel.hpp:68-85, kernel.cu:86-100)"""
        return self._eval(2, x1, x2, params)[0]


class MeanPriors(object):
    """Native-module view of the mean-function priors N(mean, cov) (bindings.cu:558-582, gppriors.hpp): constructed from a
    mean vector and a covariance MATRIX; accessor names of the pybind class.  The numbers the device needs (b, B^-1,
    B^-1 b, log|B|) come from here (DenseGP_GPU.set_mean_priors)."""

    def __init__(self, mean=(), cov=()):
        self._mean = np.reshape(np.array(mean, dtype=np.float64), (-1,))
        self._cov = np.array(cov, dtype=np.float64).reshape(self._mean.size, self._mean.size) if self._mean.size else np.zeros((0, 0))
        if self._mean.size and not np.all(np.diag(self._cov) > 0.):
            raise RuntimeError("all covariances must be greater than zero in MeanPriors")
        self.set_prior_dists()

    def set_prior_dists(self, ptypes=None, priorparams=None):
        """set_prior_dists(): one weak prior per mean parameter; set_prior_dists(types, [[shape, scale], ...]): the given
        distributions -- as in the reference they are only SAMPLED from (start points of a fit), they do not enter the
        log-posterior (gppriors.hpp:244-275)."""
        q = self.get_n_params()
        if ptypes is None:
            self._dists = [WeakPrior() for _ in range(q)]
            return
        ptypes, priorparams = list(ptypes), list(priorparams if priorparams is not None else [])
        if len(ptypes) != q or len(priorparams) != q:
            raise RuntimeError("Number of prior types and parameter sets must equal number of meanfunc parameters.")
        self._dists = [GPPriors.make_prior(t, pp) for t, pp in zip(ptypes, priorparams)]

    def sample(self, transform=None):
        """one draw per mean parameter (gppriors.hpp:277-283); weak priors draw the raw value from U(-2.5, 2.5)"""
        return [d.sample(transform) for d in self._dists]

    def get_mean(self):
        return self._mean.copy()

    def get_cov(self):
        return self._cov.copy()

    def get_n_params(self):
        return int(self._mean.size)

    def has_weak_priors(self):
        return self._mean.size == 0

    def dm_dot_b(self, dm):
        dm = np.asarray(dm, dtype=np.float64)
        return np.zeros(dm.shape[0]) if self.has_weak_priors() else dm @ self._mean

    def inv_cov(self):
        return np.zeros((0, 0)) if self.has_weak_priors() else np.linalg.inv(self._cov)

    def inv_cov_b(self):
        return np.zeros(0) if self.has_weak_priors() else np.linalg.solve(self._cov, self._mean)

    def logdet_cov(self):
        return 0. if self.has_weak_priors() else float(np.linalg.slogdet(self._cov)[1])

    def native_params(self):
        """(q, b, B^-1, B^-1 b, log|B|) for DenseGP_GPU.set_mean_priors"""
        if self.has_weak_priors():
            return 0, np.zeros(1), np.zeros(1), np.zeros(1), 0.
        return (self.get_n_params(), np.ascontiguousarray(self._mean), np.ascontiguousarray(self.inv_cov()),
                np.ascontiguousarray(self.inv_cov_b()), self.logdet_cov())


class SquaredExponentialKernel(_KernelBase):
    _kt = kernel_type.SquaredExponential


class Matern52Kernel(_KernelBase):
    _kt = kernel_type.Matern52


class ProductMat52Kernel(_KernelBase):
    _kt = kernel_type.ProductMat52


class UniformSqExpKernel(_KernelBase):
    _kt = kernel_type.UniformSqExp

    def get_n_params(self, inputs):
        return 1


class UniformMat52Kernel(UniformSqExpKernel):
    _kt = kernel_type.UniformMat52


_KERNEL_OBJECTS = {0: SquaredExponentialKernel, 1: Matern52Kernel, 2: ProductMat52Kernel, 3: UniformSqExpKernel,
                   4: UniformMat52Kernel}
