"""
Joint posterior sample paths of a fitted emulator.

A joint draw f(X*) ~ N(mu*, Sigma*) of the emulated function at a set of query points is how emulator uncertainty enters anything that is
not linear in f: the distribution of a maximum or of an exceedance area over a grid, Thompson-style selection of the next design point,
emulator uncertainty pushed through a downstream model, a plot of plausible curves.  With mu*, Sigma* what ``predict(full_cov=True)``
returns (nugget not included),

    Sigma~ = Sigma* + (include_nugget ? nugget used by the fit : 0) I + jitter I + delta I = L L^T,     samples[s] = mu* + L z[s].

Sigma* is built on the device with the launches of ``predict(full_cov=True)``, factored there by the batched Cholesky of the fit in a
scratch engine, the normals are generated there by a counter-based generator, and mu* + L z is one fp64-MFMA kernel
(``csrc/kernels_sample.hip``): only the draws cross the bus.

Jitter ladder: delta = 0 on the first try; an emulator whose Sigma~ does not factorise (Sigma* is numerically singular near training
points) is tried again with delta = mean(diag Sigma*) 1e-6 10^t, t = 0 .. 4 -- the adaptive-nugget rule of the fit applied to the
predictive covariance.  After the fifth failure the emulator has ``ok`` False and NaN samples; nothing is raised.

The generator is specified exactly (``philox_normals`` below is the same rule in NumPy): Philox4x32-10 keyed by a 64-bit seed, counter =
(point pair, draw, stream, 0), Box-Muller on 53-bit uniforms.  A value depends on (seed, stream, draw, point) alone and never on how the
work was cut; emulator e of a model draws from ``stream + e``, so that it reproduces as ``sample_posterior(single_gp_e, ..., stream=e)``.

Not covered: ``nugget="pivot"`` and ``analytic_mean=True`` (``RuntimeError``), ``dist.ShardedMultiOutputGP``, and sampling jointly over
the hyperparameters (compose with ``predict_marginal``'s samples).
"""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 of counters (..., 4) under keys (..., 2) (uint32, broadcast against each other): the output words (..., 4)"""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def philox_normals(seed, stream, n_draws, m, first_draw=0):
    """The (n_draws, m) standard normals the device generates for (seed, stream): row s, column j from counter (j >> 1, first_draw + s,
    stream, 0) under key (seed & 0xffffffff, seed >> 32); u1 = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53, u2 = ((x2 >> 5) 2^26 + (x3 >> 6))
    2^-53, r = sqrt(-2 ln u1), z[2p] = r cos(2 pi u2), z[2p + 1] = r sin(2 pi u2); an odd m drops the last sine."""
    seed, S, m = int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_draws), int(m)
    pairs = (m + 1) // 2
    ctr = np.zeros((S, pairs, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(pairs, dtype=np.uint64)[None, :]
    ctr[..., 1] = (np.arange(S, dtype=np.uint64) + np.uint64(first_draw))[:, None]
    ctr[..., 2] = np.uint64(int(stream) & 0xFFFFFFFF)
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    u1 = ((x[..., 0] >> np.uint64(5)).astype(np.float64) * 2. ** 26 + (x[..., 1] >> np.uint64(6)).astype(np.float64) + 1.) * 2. ** -53
    u2 = ((x[..., 2] >> np.uint64(5)).astype(np.float64) * 2. ** 26 + (x[..., 3] >> np.uint64(6)).astype(np.float64)) * 2. ** -53
    r, a = np.sqrt(-2. * np.log(u1)), 6.283185307179586476925286766559 * u2
    z = np.empty((S, 2 * pairs))
    z[:, 0::2], z[:, 1::2] = r * np.cos(a), r * np.sin(a)
    return np.ascontiguousarray(z[:, :m])


class PosteriorSamples(object):
    """What ``sample_posterior`` returns.  For a ``MultiOutputGP_GPU`` (for a ``GaussianProcessGPU`` without the emulator axis):

    * ``samples`` (E, S, m)     the draws; NaN where ``ok`` is False
    * ``mean`` (E, m)           the mu* they are drawn around -- the mean of ``predict(full_cov=True)``, bit for bit
    * ``ok`` (E,) bool          False where Sigma~ could not be factorised even on the last rung of the jitter ladder (or the emulator is not fit)
    * ``jitter_used`` (E,)      jitter + delta: what was added to the diagonal beyond the nugget
    * ``seed``                  the 64-bit seed of the device generator (None where ``z`` was given)
    * ``z`` (E, S, m) or None   the standard normals used (``return_z=True``)"""

    def __init__(self, samples, mean, ok, jitter_used, seed, z):
        self.samples, self.mean, self.ok, self.jitter_used, self.seed, self.z = samples, mean, ok, jitter_used, seed, z

    @property
    def n_draws(self):
        return self.samples.shape[-2]


def sample_posterior(gp, testing, n_draws=1, rng=None, z=None, include_nugget=True, jitter=0.0, stream=0, return_z=False, max_slots=0,
                     max_draws=0):
    """``n_draws`` joint draws of a fitted ``GaussianProcessGPU`` or ``MultiOutputGP_GPU`` (the multi-device form included) at ``testing``
    (m, D), computed on the device.

    ``z=None``: the normals are generated on the device from a 64-bit seed -- one ``rng.integers(0, 2**64, dtype=np.uint64)`` draw from
    ``rng`` (Generator, int seed or None), returned in ``.seed`` -- by the generator ``philox_normals`` restates; emulator e uses stream
    ``stream + e``.  ``z`` given: the caller's normals, (S, m) shared by all emulators or (n_emulators, S, m) (common random numbers,
    antithetic pairs, exact tests); ``n_draws`` is then taken from its shape.  ``return_z=True`` returns the normals used.
    ``include_nugget`` adds the nugget of the fit to the diagonal, ``jitter`` a constant of the caller's; the jitter ladder of the module
    docstring is applied on top where the factorisation fails.  ``max_slots`` / ``max_draws`` bound the emulators per pass and the draws per
    chunk (0: the library's choice); ``max_draws`` changes no bit of the result.

    Every argument is checked before the device is touched.  ``RuntimeError`` for ``nugget="pivot"``, ``analytic_mean=True`` and a
    ``GaussianProcessGPU`` that is not fit; emulators of a ``MultiOutputGP_GPU`` that are not fit give NaN rows with ``ok`` False.
    Returns a ``PosteriorSamples``."""
    from . import LibGPGPU
    if not LibGPGPU.HAVE_LIBGPGPU:
        raise TypeError("sample_posterior needs a GaussianProcessGPU or a MultiOutputGP_GPU (the device library is not loaded)")
    from .GaussianProcessGPU import GaussianProcessGPU
    from .MultiOutputGP_GPU import MultiOutputGP_GPU
    if not isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)):
        raise TypeError("sample_posterior needs a GaussianProcessGPU or a MultiOutputGP_GPU")
    single = isinstance(gp, GaussianProcessGPU)
    D = int(gp.D)
    testing = np.ascontiguousarray(testing, dtype=np.float64)
    if testing.ndim == 1:
        testing = testing.reshape(-1, 1) if D == 1 else testing.reshape(1, -1)
    if testing.ndim != 2 or testing.shape[1] != D or testing.shape[0] < 1:
        raise ValueError("sample_posterior: testing must have shape (m, D) with D = %d and at least one point" % D)
    if not np.all(np.isfinite(testing)):
        raise ValueError("sample_posterior: testing must be finite")
    m = testing.shape[0]
    if not (float(jitter) >= 0. and np.isfinite(float(jitter))):
        raise ValueError("sample_posterior: jitter must be a finite number that is not negative")
    if int(max_slots) < 0 or int(max_draws) < 0:
        raise ValueError("sample_posterior: max_slots and max_draws must not be negative")
    if int(stream) < 0 or int(stream) >= 2 ** 32:
        raise ValueError("sample_posterior: stream must be in [0, 2^32)")
    ne = None if single else int(gp.n_emulators)
    if z is not None:
        z = np.ascontiguousarray(z, dtype=np.float64)
        shared = z.ndim == 2 and z.shape[1] == m
        per = (not single) and z.ndim == 3 and z.shape[0] == ne and z.shape[2] == m
        if not (shared or per) or z.shape[-2] < 1:
            raise ValueError("sample_posterior: z must have shape (n_draws, m)%s with m = %d"
                             % ("" if single else " or (n_emulators, n_draws, m)", m))
        if not np.all(np.isfinite(z)):
            raise ValueError("sample_posterior: z must be finite")
        S = z.shape[-2]
    else:
        S = int(n_draws)
        if S < 1:
            raise ValueError("sample_posterior: n_draws must be at least 1")
    pivot = gp.nugget_type == "pivot" if single else gp._nugget_name == "pivot"
    if pivot:
        raise RuntimeError("sample_posterior: not available with nugget=\"pivot\"")
    if getattr(gp, "_analytic_mean", False):
        raise RuntimeError("sample_posterior: not available with analytic_mean=True")
    native = gp._densegp_gpu if single else gp._mogp_gpu
    if single and not native.theta_fit_status():
        raise RuntimeError("sample_posterior: hyperparameters have not been fit for this Gaussian Process")
    seed = None
    if z is None:
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        seed = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
    samples, mean, zout, ju, ok = native.sample_posterior(testing, n_draws=S, seed=seed or 0, stream=int(stream), z=z,
                                                         include_nugget=include_nugget, jitter=float(jitter), max_slots=int(max_slots),
                                                         max_draws=int(max_draws), return_z=bool(return_z))
    return PosteriorSamples(samples=samples, mean=mean, ok=ok, jitter_used=ju, seed=seed, z=zout)
