"""
Local approximate GP prediction for designs far beyond what one dense factorisation holds (Emery 2009; Gramacy & Apley 2015, "laGP").

The hyperparameters are fitted once, on a subsample the dense path can handle (a ``GaussianProcessGPU`` or a ``MultiOutputGP_GPU``).  Every
query point is then predicted from the GP on its k nearest design points alone -- nearest in the metric the fitted correlation lengths
define -- at those hyperparameters:

    s_d = sqrt(exp(theta_d))                              (one shared value for the uniform kernels)
    r2(x, q) = sum_d (x_d s_d - q_d s_d)^2                the scaled squared distance
    Q = sigma^2 k(r2) + (nugget + jitter) I               over the k neighbours of q,  Q = L L^T
    mean = m(q) + k*^T Q^-1 (y - m(X)),    unc = max(sigma^2 - |L^-1 k*|^2 + nugget, 0)

The work is m independent k x k problems, k <= 126: a brute-force neighbour search and one 128 x 128 factorisation per query, both on the
device (``csrc/kernels_local.hip``).  The design and the mean-subtracted targets go up once and stay there for every ``predict``.

The neighbour search is exact and reproducible: the device forms x_d * s_d and q_d * s_d (one rounded multiply each) and
r2 = ((0 + t_0 t_0) + t_1 t_1) + ... with t_d their difference, in the order d = 0 .. D-1 and without fused multiply-add, so NumPy gives
the same bits; the neighbours are the k smallest pairs (r2, index) in lexicographic order, ties to the lowest index.

Not covered: ``nugget="pivot"``, ``analytic_mean=True``, ``ProductMat52`` (not a function of one r2), k > 126, ALC-greedy local designs,
local re-estimation of the hyperparameters, an adaptive nugget for queries whose local matrix is not positive definite (``jitter=`` is the
caller's tool, ``n_failed`` says when to use it), search trees, derivatives, and one ``LocalGP`` spread over several devices.
"""
import numpy as np

MAX_NEIGHBOURS = 126         # the neighbours, the target row and the query row share one 128 x 128 tile
MAX_D = 80
_KERNELS = {"SquaredExponential": (0, False), "Matern52": (1, False), "UniformSqExp": (0, True), "UniformMat52": (1, True)}


class LocalPrediction(object):
    """What ``LocalGP.predict`` returns (shapes (m,) for a ``GaussianProcessGPU``, (E, m) for a ``MultiOutputGP_GPU``):

    * ``mean``, ``unc``      predictive mean and variance; ``unc`` is None with ``unc=False``; NaN where ``ok`` is False
    * ``ok``                 bool: the local matrix of that query was positive definite
    * ``radius``             the scaled squared distance of the k-th neighbour
    * ``neighbours``         (m, k) / (E, m, k) int64 design indices, nearest first, with ``return_neighbours=True``; else None
    * ``n_failed``           the number of False flags in ``ok``"""

    def __init__(self, mean, unc, ok, radius, neighbours):
        self.mean, self.unc, self.ok, self.radius, self.neighbours = mean, unc, ok, radius, neighbours

    @property
    def n_failed(self):
        return int(np.size(self.ok) - np.count_nonzero(self.ok))


def _points(name, who, x, D):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1) if D == 1 else x.reshape(1, -1)
    if x.ndim != 2 or x.shape[1] != D or x.shape[0] < 1:
        raise ValueError("%s: %s must have shape (m, D) with D = %d and at least one point" % (who, name, D))
    if not np.all(np.isfinite(x)):
        raise ValueError("%s: %s must be finite" % (who, name))
    return x


def _emulator_type(who, gp):
    from . import LibGPGPU
    if not LibGPGPU.HAVE_LIBGPGPU:
        raise TypeError("%s needs a GaussianProcessGPU or a MultiOutputGP_GPU (the device library is not loaded)" % who)
    from .GaussianProcessGPU import GaussianProcessGPU
    from .MultiOutputGP_GPU import MultiOutputGP_GPU
    if not isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)):
        raise TypeError("%s needs a GaussianProcessGPU or a MultiOutputGP_GPU" % who)
    return isinstance(gp, GaussianProcessGPU)


def _fit_state(who, gp, single):
    """the refusals that need no device; returns the native emulators the hyperparameters are read from"""
    pivot = gp.nugget_type == "pivot" if single else gp._nugget_name == "pivot"
    if pivot:
        raise RuntimeError("%s: not available with nugget=\"pivot\"" % who)
    if getattr(gp, "_analytic_mean", False):
        raise RuntimeError("%s: not available with analytic_mean=True" % who)
    natives = [gp._densegp_gpu] if single else [gp._mogp_gpu.emulator(i) for i in range(int(gp.n_emulators))]
    for i, em in enumerate(natives):
        if not em.theta_fit_status():
            raise RuntimeError("%s: hyperparameters have not been fit for %s" % (who, "this Gaussian Process" if single else "emulator %d" % i))
    for em in natives:
        name = str(em.get_kernel_type()).split(".")[1]
        if name not in _KERNELS:
            raise RuntimeError("%s: not available with the %s kernel (not a function of one scaled distance)" % (who, name))
    return natives


def _hyperparameters(em, D):
    """what the device needs of one fitted native emulator: (kernel 0 / 1, s (D,), sigma^2, nugget, mean function, its parameters)"""
    kt, uniform = _KERNELS[str(em.get_kernel_type()).split(".")[1]]
    th = em.get_theta()
    corr = np.asarray(th.get_corr_raw(), dtype=np.float64)
    s = np.sqrt(np.exp(corr))
    s = np.full(D, s[0]) if uniform else np.ascontiguousarray(s)
    if s.shape != (D,) or not np.all(np.isfinite(s)) or not np.all(s > 0.):
        raise RuntimeError("predict_local: the correlation parameters do not give %d positive finite scales" % D)
    return kt, s, float(th.get_cov()), float(em.get_nugget_size()), em.get_meanfunc(), np.asarray(th.get_mean(), dtype=np.float64)


def _mean_at(meanfunc, params, x):
    if meanfunc is None or (meanfunc.get_n_params() == 0 and type(meanfunc).__name__ == "ZeroMeanFunc"):
        return np.zeros(x.shape[0])
    return np.asarray(meanfunc.mean_f(x, params), dtype=np.float64).reshape(x.shape[0])


def _create_native(inputs, residuals, device):
    from . import LibGPGPU
    return LibGPGPU.LocalGP_GPU(inputs, residuals, device=device)


class LocalGP(object):
    """``LocalGP(gp, inputs, targets, n_neighbours=50, device=None)``

    ``gp``: a fitted ``GaussianProcessGPU`` (E = 1) or ``MultiOutputGP_GPU`` (E emulators), used only as the source of the kernel, the
    hyperparameters (correlation parameters, sigma^2 and the nugget as ``gp.nugget`` / ``get_nugget_size()`` report it) and the mean
    function; its own training set is typically a subsample, and it is never modified.  ``inputs`` (N, D) and ``targets`` (N,) or (E, N):
    the whole design, N far beyond what the dense path holds (N < 2^31 - 256: design indices are 32-bit, element offsets 64-bit).  The mean
    function is evaluated here at ``inputs`` and subtracted; the device sees residuals only.  ``device=None``: the current device.

    Every argument is checked before the device is touched.  ``RuntimeError`` for ``nugget="pivot"``, ``analytic_mean=True``,
    ``ProductMat52`` and an emulator that is not fit; ``ValueError`` for shapes, non-finite values and ``n_neighbours`` outside
    1 .. min(N, 126).  The native handle is freed by ``close()`` (and on deletion)."""

    def __init__(self, gp, inputs, targets, n_neighbours=50, device=None):
        who = "LocalGP"
        self._native = None
        single = _emulator_type(who, gp)
        D = int(gp.D)
        if D > MAX_D:
            raise ValueError("%s: at most %d input dimensions" % (who, MAX_D))
        inputs = _points("inputs", who, inputs, D)
        N = inputs.shape[0]
        if N >= 2 ** 31 - 256:
            raise ValueError("%s: the design must have fewer than 2^31 - 256 points" % who)
        natives = _fit_state(who, gp, single)
        E = len(natives)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.shape != ((N,) if single else (E, N)) and not (E == 1 and targets.shape in ((N,), (1, N))):
            raise ValueError("%s: targets must have shape %s" % (who, "(N,) with N = %d" % N if single else "(E, N) with E = %d, N = %d" % (E, N)))
        targets = targets.reshape(E, N)
        if not np.all(np.isfinite(targets)):
            raise ValueError("%s: targets must be finite" % who)
        k = int(n_neighbours)
        if k != n_neighbours or k < 1 or k > min(N, MAX_NEIGHBOURS):
            raise ValueError("%s: n_neighbours must be between 1 and min(N, %d) = %d" % (who, MAX_NEIGHBOURS, min(N, MAX_NEIGHBOURS)))
        if device is not None and (int(device) != device or int(device) < 0):
            raise ValueError("%s: device must be a device ordinal or None" % who)
        self._single, self._D, self._N, self._E, self._k = single, D, N, E, k
        self._hyper = [_hyperparameters(em, D) for em in natives]
        resid = np.stack([targets[e] - _mean_at(h[4], h[5], inputs) for e, h in enumerate(self._hyper)])
        self._native = _create_native(inputs, np.ascontiguousarray(resid), None if device is None else int(device))

    @classmethod
    def _on_handle(cls, native, hyper, D, N, n_neighbours):
        """Internal: a single-output view on a native handle that somebody else owns (``VecchiaGP.predict``), at the hyperparameters
        ``hyper`` = [(kernel 0 / 1, s (D,), sigma^2, nugget, mean function or None, its parameters)] in place of a fitted ``gp``.
        ``close()`` of the view leaves the handle open."""
        who = "LocalGP"
        k = int(n_neighbours)
        if k != n_neighbours or k < 1 or k > min(N, MAX_NEIGHBOURS):
            raise ValueError("%s: n_neighbours must be between 1 and min(N, %d) = %d" % (who, MAX_NEIGHBOURS, min(N, MAX_NEIGHBOURS)))
        self = cls.__new__(cls)
        self._single, self._D, self._N, self._E, self._k = True, int(D), int(N), 1, k
        self._hyper, self._native, self._borrowed = list(hyper), native, True
        return self

    n_neighbours = property(lambda self: self._k)
    n = property(lambda self: self._N)
    D = property(lambda self: self._D)
    n_emulators = property(lambda self: self._E)

    def close(self):
        native, self._native = getattr(self, "_native", None), None
        if native is not None and not getattr(self, "_borrowed", False):
            native.close()

    def __del__(self):
        self.close()

    def predict(self, testing, unc=True, include_nugget=True, jitter=0.0, return_neighbours=False, max_points=0):
        """Predict at ``testing`` (m, D) from the ``n_neighbours`` nearest design points of every query; returns a ``LocalPrediction``.

        ``include_nugget``: add the nugget to ``unc`` as ``predict`` of the emulator does.  ``jitter`` >= 0 is added to the diagonal of
        every local matrix (not to ``unc``): the tool for queries whose matrix is not positive definite (``ok`` False, NaN in that row,
        counted by ``n_failed``; no other row is affected).  ``max_points`` caps the queries per device pass (0: sized by the free device
        memory) and changes no bit of the result.  Emulator e of a ``MultiOutputGP_GPU`` uses its own hyperparameters, hence its own
        metric and neighbours; the emulators run one after another on the same handle."""
        who = "LocalGP.predict"
        testing = _points("testing", who, testing, self._D)
        jitter = float(jitter)
        if not (jitter >= 0. and np.isfinite(jitter)):
            raise ValueError("%s: jitter must be a finite number that is not negative" % who)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        if self._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        rows = []
        for e, (kt, s, sigma2, nugget, meanfunc, mparams) in enumerate(self._hyper):
            mean, var, ok, radius, nbr = self._native.predict(e, kt, s, sigma2, nugget, jitter, include_nugget, testing, self._k,
                                                              max_points=int(max_points), unc=bool(unc),
                                                              return_neighbours=bool(return_neighbours))
            mean += _mean_at(meanfunc, mparams, testing)
            rows.append((mean, var, ok, radius, nbr))
        if self._single:
            return LocalPrediction(*rows[0])
        cols = list(zip(*rows))
        return LocalPrediction(np.stack(cols[0]), np.stack(cols[1]) if unc else None, np.stack(cols[2]), np.stack(cols[3]),
                               np.stack(cols[4]) if return_neighbours else None)


def predict_local(gp, inputs, targets, testing, n_neighbours=50, **predict_kwargs):
    """One-shot form: ``LocalGP(gp, inputs, targets, n_neighbours).predict(testing, **predict_kwargs)``; the handle is freed afterwards."""
    device = predict_kwargs.pop("device", None)
    lg = LocalGP(gp, inputs, targets, n_neighbours=n_neighbours, device=device)
    try:
        return lg.predict(testing, **predict_kwargs)
    finally:
        lg.close()
