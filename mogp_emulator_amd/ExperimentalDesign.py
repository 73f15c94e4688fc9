"""
One-shot experimental designs -- counterpart of mogp_emulator/ExperimentalDesign.py (``ExperimentalDesign``, ``MonteCarloDesign``,
``LatinHypercubeDesign``, ``MaxiMinLHC``), written from its behaviour.

A design holds one probability point function (PPF: [0, 1] -> parameter value) per parameter.  ``sample(n)`` draws n points of the
unit hypercube with the class's ``_draw_samples`` and maps every column through its PPF.

Monte-Carlo and Latin-hypercube draws are host work and consume the legacy global ``np.random`` stream in the reference's order (per
hypercube: one shuffle per parameter, then one ``random((n, D))``), so a seeded run returns the reference's design bit for bit.  These
two classes need neither the library nor a device.

``MaxiMinLHC`` keeps, of ``n_tries`` hypercubes, the first with the largest minimum pairwise distance.  The reference runs
``scipy.spatial.distance.pdist`` on one try after the other; here the tries are drawn on the host in the same order and scored in
chunks by one device call each (``libgpgpu.design_min_pdist``, csrc/kernels_design.hip).  There is no CPU fallback for that path
(DESIGN.md section 1): without the library or a device ``MaxiMinLHC`` raises as ``GaussianProcessGPU`` does.  Only a ``pdist`` keyword
(``metric=...``) is served by scipy on the host, because the device kernel computes the default Euclidean metric only.
"""
from inspect import signature

import numpy as np
import scipy.stats

from . import LibGPGPU


def _as_bounds(pair):
    """(lo, hi) floats of a two-number iterable with lo < hi; None when `pair` is not two numbers."""
    if len(pair) != 2:
        return None
    lo, hi = float(pair[0]), float(pair[1])
    if hi <= lo:
        raise ValueError("bad value for parameter bounds in ExperimentalDesign")
    return lo, hi


def _uniform_ppf(lo, hi):
    return scipy.stats.uniform(loc=lo, scale=hi - lo).ppf


def _checked_ppf(fn):
    if len(signature(fn).parameters) != 1:
        raise ValueError("PPF distribution provided must accept a single argument")
    return fn


class ExperimentalDesign(object):
    """Base class: the parameter distributions and the PPF mapping.  Accepted arguments: ``(n)`` -- n parameters uniform on [0, 1];
    ``(n, (a, b))`` -- uniform on [a, b]; ``(n, ppf)`` -- one PPF for all; ``([(a, b), ...])`` or ``([ppf, ...])`` -- one entry
    per parameter.  A derived class provides ``_draw_samples(n_samples, **kwargs)`` and sets ``self.method``."""

    def __init__(self, *args):
        if len(args) not in (1, 2):
            raise ValueError("bad inputs for ExperimentalDesign")
        spec = None
        try:
            n_parameters = int(args[0])
        except TypeError:
            if len(args) == 2:
                raise TypeError("bad input type for ExperimentalDesign")
            try:
                spec = list(args[0])
            except TypeError:
                raise TypeError("bad input type for ExperimentalDesign")
            n_parameters = len(spec)
        if len(args) == 2:
            if callable(args[1]):
                spec = args[1]
            else:
                try:
                    spec = list(args[1])
                except TypeError:
                    raise TypeError("bad input type for ExperimentalDesign")
                try:
                    pair = _as_bounds(spec)
                except TypeError:           # entries that are no numbers: a per-parameter list
                    pair = None
                if pair is not None:
                    spec = pair
        if n_parameters <= 0:
            raise ValueError("number of parameters must be positive in Experimental Design")
        self.n_parameters = n_parameters

        if spec is None:
            self.distributions = [_uniform_ppf(0., 1.)] * n_parameters
        elif isinstance(spec, tuple):
            self.distributions = [_uniform_ppf(*spec)] * n_parameters
        elif callable(spec):
            self.distributions = [_checked_ppf(spec)] * n_parameters
        else:
            if len(spec) != n_parameters:
                raise ValueError("list of parameter distributions must have the same length")
            self.distributions = []
            for item in spec:
                if callable(item):
                    self.distributions.append(_checked_ppf(item))
                    continue
                try:
                    pair = _as_bounds(item)
                except TypeError:
                    raise TypeError("bounds for each parameter must be a tuple of two floats")
                if pair is None:
                    raise ValueError("bounds for each parameter must be a tuple of two floats")
                self.distributions.append(_uniform_ppf(*pair))

    def get_n_parameters(self):
        return self.n_parameters

    def get_method(self):
        try:
            return self.method
        except AttributeError:
            raise NotImplementedError("base class of ExperimentalDesign does not implement a method")

    def _draw_samples(self, n_samples):
        raise NotImplementedError

    def sample(self, n_samples, **kwargs):
        """(n_samples, n_parameters) points of the parameter space; keywords go to ``_draw_samples``."""
        n_samples = int(n_samples)
        assert n_samples > 0, "number of samples must be positive"
        unit = self._draw_samples(n_samples, **kwargs)
        assert np.all(unit >= 0.) and np.all(unit <= 1.), "error in generating random samples"
        values = np.zeros((n_samples, self.get_n_parameters()))
        for col, ppf in enumerate(self.distributions):
            for row in range(n_samples):                 # one call per value: a PPF need not accept arrays
                values[row, col] = ppf(unit[row, col])
        assert np.all(np.isfinite(values)), "error due to non-finite values of parameters"
        return values

    def __str__(self):
        try:
            prefix = self.get_method() + " "
        except NotImplementedError:
            prefix = ""
        return prefix + "Experimental Design with " + str(self.get_n_parameters()) + " parameters"


class MonteCarloDesign(ExperimentalDesign):
    """Independent uniform draws of the unit hypercube."""

    def __init__(self, *args):
        self.method = "Monte Carlo"
        super().__init__(*args)

    def _draw_samples(self, n_samples, **kwargs):
        n_samples = int(n_samples)
        assert n_samples > 0, "number of samples must be positive"
        return np.random.random((n_samples, self.get_n_parameters()))


class LatinHypercubeDesign(ExperimentalDesign):
    """Latin hypercube: every parameter has exactly one sample in each of its n_samples equal-probability strata."""

    def __init__(self, *args):
        self.method = "Latin Hypercube"
        super().__init__(*args)

    def _draw_samples(self, n_samples, **kwargs):
        n_samples = int(n_samples)
        assert n_samples > 0, "number of samples must be positive"
        out = np.empty((n_samples, self.get_n_parameters()))
        self._draw_into(out)
        assert np.all(out >= 0.) and np.all(out <= 1.), "error in generating latin hypercube samples"
        return out

    def _draw_into(self, out):
        """One hypercube into out (n, D).  Order of the random stream: a shuffle of the strata per parameter, then the offsets inside
        the strata as one (n, D) block."""
        n, D = out.shape
        strata = np.empty((D, n))
        for d in range(D):
            strata[d] = np.arange(n, dtype=np.float64) / float(n)
            np.random.shuffle(strata[d])
        np.add(strata.T, np.random.random((n, D)) / float(n), out=out)


class MaxiMinLHC(LatinHypercubeDesign):
    """Of ``n_tries`` Latin hypercubes, the one whose closest pair of points is furthest apart (the first such one on a tie)."""

    # host memory for the tries of one device call; the kept design does not depend on it
    CHUNK_BYTES = 256 << 20

    def __init__(self, *args):
        # get_method() answers "Latin Hypercube", as the reference's MaxiMinLHC does (there the parent's constructor overwrites the name)
        super().__init__(*args)

    def _draw_samples(self, n_samples, n_tries=1000, **kwargs):
        n_samples = int(n_samples)
        assert n_samples > 0, "number of samples must be positive"
        assert n_tries > 0, "n_tries must be a positive integer"
        n_tries = int(n_tries)
        D = self.get_n_parameters()
        on_device = not kwargs
        if on_device:
            if not LibGPGPU.HAVE_LIBGPGPU:
                raise RuntimeError("Cannot draw a MaxiMinLHC: The GPU library (libgpgpu) could not be loaded")
            if not LibGPGPU.gpu_usable():
                raise RuntimeError("Cannot draw a MaxiMinLHC: A compatible GPU could not be found")
            score = LibGPGPU.design_min_pdist
        else:
            from scipy.spatial.distance import pdist

            def score(tries):
                return np.array([np.min(pdist(t, **kwargs)) for t in tries])

        per_call = int(max(1, min(n_tries, self.CHUNK_BYTES // (8 * n_samples * D))))
        tries = np.empty((per_call, n_samples, D))
        best, best_dist = np.empty((n_samples, D)), -np.inf
        for t0 in range(0, n_tries, per_call):
            nb = min(per_call, n_tries - t0)
            for t in range(nb):
                self._draw_into(tries[t])
            dist = score(tries[:nb])
            if np.all(np.isnan(dist)):
                continue
            k = int(np.nanargmax(dist))             # the first try of the chunk with its largest distance; a NaN never wins
            if dist[k] > best_dist:
                best_dist = dist[k]
                best = tries[k].copy()
        assert np.all(best >= 0.0) and np.all(best <= 1.0), "error in generating latin hypercube samples"
        return best
