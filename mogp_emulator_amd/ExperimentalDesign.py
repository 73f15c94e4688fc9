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

``OptimisedLHC`` searches instead of drawing again: ``n_chains`` independent chains of column-swap threshold accepting on Morris &
Mitchell's criterion run on the device (``libgpgpu.design_anneal_lhs``, csrc/kernels_lhs.hip; DESIGN.md section 3 "Design"), and the chain
whose closest pair is furthest apart is kept.  It has no CPU fallback either.
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


class OptimisedLHC(LatinHypercubeDesign):
    """A maximin Latin hypercube found by search: from ``n_chains`` random hypercubes, each chain exchanges two entries of one column at a
    time and keeps the exchange when Morris & Mitchell's criterion (q = 5: p = 10 on distances) does not rise above a shrinking threshold;
    of the chains' best states, the one with the largest minimum distance wins (then the fewest pairs at it, then the first chain).

    ``sample(n_samples, n_chains=64, n_steps=None, q=5, theta0=0.1, rho=0.9, offsets="centre", seed=None, start=None, return_info=False)``

    * the chain starts come from the legacy ``np.random`` stream: per chain one shuffle per parameter, in the parent's order; then, with
      ``seed=None``, the 64-bit seed of the device's counter-based generator (two 32-bit draws, low word first) -- so ``np.random.seed(s)``
      fixes the whole result;
    * ``offsets="centre"`` puts point i at (P_i + 1/2) / n; ``"random"`` adds one ``np.random.random((n, D)) / n`` block after the search,
      as the parent does;
    * ``start``: a level matrix (n, D) or several (C, n, D) of the caller (every column a permutation of 0 .. n-1) to polish, in place of the
      random starts (``n_chains`` is then their number);
    * ``n_steps=None``: ``STEPS_PER_CELL * n_samples * n_parameters`` proposals per chain (DESIGN.md section 3 "Design" has the scan behind it);
    * ``return_info=True``: also a dict with the per-chain ``phi``, ``min_r``, ``pairs``, ``accepted``, the ``winner`` and the ``seed``."""

    STEPS_PER_CELL = 15

    def __init__(self, *args):
        # get_method() answers "Latin Hypercube", as MaxiMinLHC's does
        super().__init__(*args)

    def sample(self, n_samples, n_chains=64, n_steps=None, q=5, theta0=0.1, rho=0.9, offsets="centre", seed=None, start=None,
               return_info=False):
        values = super().sample(n_samples, n_chains=n_chains, n_steps=n_steps, q=q, theta0=theta0, rho=rho, offsets=offsets, seed=seed,
                                start=start)
        return (values, self._info) if return_info else values

    def _draw_samples(self, n_samples, n_chains=64, n_steps=None, q=5, theta0=0.1, rho=0.9, offsets="centre", seed=None, start=None):
        n = int(n_samples)
        assert n > 0, "number of samples must be positive"
        D = self.get_n_parameters()
        if offsets not in ("centre", "random"):
            raise ValueError("offsets must be 'centre' or 'random'")
        if not LibGPGPU.HAVE_LIBGPGPU:
            raise RuntimeError("Cannot draw an OptimisedLHC: The GPU library (libgpgpu) could not be loaded")
        if not LibGPGPU.gpu_usable():
            raise RuntimeError("Cannot draw an OptimisedLHC: A compatible GPU could not be found")
        if start is None:
            n_chains = int(n_chains)
            assert n_chains > 0, "n_chains must be a positive integer"
            levels = np.empty((n_chains, n, D), dtype=np.int32)
            column = np.empty(n, dtype=np.int32)
            for c in range(n_chains):
                for d in range(D):
                    column[:] = np.arange(n)
                    np.random.shuffle(column)
                    levels[c, :, d] = column
        else:
            levels = np.asarray(start)
            if levels.ndim == 2:
                levels = levels[None]
            if levels.ndim != 3 or levels.shape[1:] != (n, D):
                raise ValueError("start must have shape (n_samples, n_parameters) or (n_chains, n_samples, n_parameters)")
        if seed is None:
            lo, hi = (int(w) for w in np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64))
            seed = lo | (hi << 32)
        seed = int(seed)
        if n_steps is None:
            n_steps = self.STEPS_PER_CELL * n * D
        if n == 1:                      # one point: nothing to exchange
            best = np.zeros((1, D), dtype=np.int32)
            self._info = dict(phi=np.zeros(1), min_r=np.zeros(1, dtype=np.int64), pairs=np.zeros(1, dtype=np.int64),
                              accepted=np.zeros(1, dtype=np.int64), winner=0, seed=seed)
        else:
            res = LibGPGPU.design_anneal_lhs(levels, n_steps, q=q, theta0=theta0, rho=rho, seed=seed)
            best = res.levels[res.winner]
            self._info = dict(phi=res.phi, min_r=res.min_r, pairs=res.pairs, accepted=res.accepted, winner=res.winner, seed=seed)
        if offsets == "centre":
            out = (best + 0.5) / float(n)
        else:
            out = best / float(n) + np.random.random((n, D)) / float(n)
        assert np.all(out >= 0.0) and np.all(out <= 1.0), "error in generating latin hypercube samples"
        return out
