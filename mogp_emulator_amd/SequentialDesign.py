"""
Sequential designs -- counterpart of mogp_emulator/SequentialDesign.py: the driver classes ``SequentialDesign`` (bookkeeping of inputs,
targets and candidates, simulator binding, save / load), ``MICEDesign`` (Mutual Information for Computer Experiments) with the MICE
candidate scoring it rests on, and ``ALCDesign`` (the integrated-variance criterion of ActiveLearning.py).

``MICEDesign._eval_metric`` (mogp_emulator/SequentialDesign.py:884-964) scores every candidate point c by

    criterion(c) = Var_base[f(c)] / Var_cand\\c[f(c)]

where the denominator is the predictive variance at c of a GP conditioned on all OTHER candidates
(``MICEFastGP.fast_predict``, :705-747; nugget = base nugget * nugget_s).  The reference evaluates the
denominator one candidate at a time, each time re-solving for the full inverse (O(n_cand^3) per
candidate) and downdating it with the Woodbury identity.  The downdated quadratic form has the closed
value 1 / [K^-1]_cc, so here ALL denominators come from one batched device factorisation + one pass
over L^-1 (``loo_variance``), and the numerator from one batched predictive-variance call.

``MICEDesign`` fits a ``GaussianProcessGPU`` to the current design at every step and calls ``mice_criterion`` once for all candidates,
so ``n_cand`` in the thousands costs about what the reference's default of 50 does.  ``SequentialDesign`` itself is host bookkeeping
and uses no device, but lives in this module, which imports the library: the package exports both classes only when the library loads.
"""
from inspect import signature

import numpy as np

from . import LibGPGPU
from .ExperimentalDesign import ExperimentalDesign
from .GaussianProcessGPU import GaussianProcessGPU
from .Priors import GPPriors
from .fitting import fit_GP_MAP


class MICEFastGP(GaussianProcessGPU):
    """GaussianProcessGPU with ``fast_predict(index)``: leave-one-out predictive variance at a training input."""

    def loo_variance(self):
        if not self.theta.data_has_been_set():
            raise ValueError("hyperparameters have not been fit for this Gaussian Process")
        return self._densegp_gpu.loo_variance()

    def fast_predict(self, index):
        index = int(index)
        assert 0 <= index < self.n, "index must be 0 <= index < n"
        key = tuple(self.theta.get_data())
        if getattr(self, "_loo_key", None) != key:
            self._loo, self._loo_key = self.loo_variance(), key
        return np.array([self._loo[index]])


def mice_criterion(gp, candidates, nugget_s=1.):
    """MICE criterion of every candidate for the fitted base emulator ``gp`` (a GaussianProcessGPU):
    returns (scores (n_cand,), index of the best candidate)."""
    candidates = np.ascontiguousarray(candidates, dtype=np.float64)
    if candidates.ndim == 1:
        candidates = candidates.reshape(-1, 1)
    assert candidates.ndim == 2 and candidates.shape[1] == gp.D, "bad shape for candidates"
    assert nugget_s >= 0., "nugget_s must be non-negative"
    if not gp.theta.data_has_been_set():
        raise ValueError("hyperparameters have not been fit for this Gaussian Process")
    n_cand, D = candidates.shape
    _, unc_base, _ = gp.predict(candidates, unc=True, deriv=False)
    fast = MICEFastGP(candidates, np.ones(n_cand), kernel=gp.kernel, nugget=float(gp.nugget * nugget_s),
                      priors=GPPriors(n_corr=D, nugget_type="fixed"), max_batch_size=max(n_cand, 1))
    fast.fit(np.asarray(gp.theta.get_data())[:D + 1])             # correlation lengths and covariance of the base fit
    scores = unc_base / fast.loo_variance()
    assert np.all(np.isfinite(scores)), "error in computing MICE critera"
    return scores, int(np.argmax(scores))


def _none_or_array(entry):
    """An entry of a saved design: None was stored as a 0-d object array."""
    arr = np.array(entry)
    if arr.dtype == object and arr.ndim == 0 and arr.item() is None:
        return None
    return arr


class SequentialDesign(object):
    """Base class of a sequential design: an initial one-shot design of ``n_init`` points drawn from ``base_design``, then one point at
    a time, each the best of ``n_cand`` fresh candidates under the metric a derived class implements (``_eval_metric`` returns the
    index of the chosen candidate).  With a bound simulator ``f`` (one array argument) the design can run itself
    (``run_sequential_design``); without one the caller alternates ``get_next_point`` / ``set_next_target`` (or the batch forms)."""

    def __init__(self, base_design, f=None, n_samples=None, n_init=10, n_cand=50):
        if not isinstance(base_design, ExperimentalDesign):
            raise TypeError("base design must be a one-shot experimental design")
        if f is not None:
            if not callable(f):
                raise TypeError("simulator f must be a function or other callable")
            if len(signature(f).parameters) != 1:
                raise ValueError("simulator f must accept all parameters as a single input array")
        if n_samples is not None and int(n_samples) < 0:
            raise ValueError("number of samples must be nonzero")
        if int(n_init) <= 0:
            raise ValueError("number of initial design points must be positive")
        if int(n_cand) <= 0:
            raise ValueError("number of candidate design points must be positive")
        self.base_design = base_design
        self.f = f
        self.n_samples = None if n_samples is None else int(n_samples)
        self.n_init = int(n_init)
        self.n_cand = int(n_cand)
        self.current_iteration = 0
        self.initialized = False
        self.inputs = None
        self.targets = None
        self.candidates = None

    # -- persistence ----------------------------------------------------------------------------------
    def save_design(self, filename):
        """inputs, targets and candidates (None included) as a numpy .npz archive."""
        np.savez(filename, inputs=self.inputs, targets=self.targets, candidates=self.candidates)

    def load_design(self, filename):
        """Restore what ``save_design`` wrote; the iteration count follows the number of targets."""
        with np.load(filename, allow_pickle=True) as archive:
            self.inputs = _none_or_array(archive["inputs"])
            self.targets = _none_or_array(archive["targets"])
            self.candidates = _none_or_array(archive["candidates"])
        if self.inputs is None:
            assert self.targets is None, "Cannot have targets without corresponding inputs"
        else:
            if self.targets is not None:
                assert self.targets.ndim == 1, "bad number of dimensions for targets"
                assert self.targets.shape[0] <= self.inputs.shape[0], "targets cannot be longer than inputs"
                self.initialized = True
                self.current_iteration = self.targets.shape[0]
            assert self.get_n_parameters() == self.inputs.shape[1], "Bad shape for inputs"
            # fewer saved points than n_init.  (The reference compares the number of PARAMETERS here, SequentialDesign.py:179, and so
            # shrinks n_init of any design with fewer parameters than initial points: a slip, not mirrored.)
            if self.inputs.shape[0] < self.n_init:
                print("n_init greater than number of inputs, changing n_init")
                self.n_init = self.inputs.shape[0]
        if self.candidates is not None:
            assert self.get_n_parameters() == self.candidates.shape[1], "Bad shape for candidates"
            if self.candidates.shape[0] != self.n_cand:
                print("shape of candidates differs from n_cand, candidates will be overridden")

    # -- getters ----------------------------------------------------------------------------------------
    def has_function(self):
        return self.f is not None

    def get_n_parameters(self):
        return self.base_design.get_n_parameters()

    def get_n_init(self):
        return self.n_init

    def get_n_samples(self):
        return self.n_samples

    def get_n_cand(self):
        return self.n_cand

    def get_current_iteration(self):
        return self.current_iteration

    def get_inputs(self):
        return self.inputs

    def get_targets(self):
        return self.targets

    def get_candidates(self):
        return self.candidates

    def get_base_design(self):
        return type(self.base_design).__name__

    # -- initial design -----------------------------------------------------------------------------------
    def generate_initial_design(self):
        assert not self.initialized, "initial design has already been created"
        self.inputs = self.base_design.sample(self.n_init)
        self.current_iteration = self.n_init
        return self.inputs

    def set_initial_targets(self, targets):
        if self.inputs is None:
            raise ValueError("Initial design has not been generated")
        assert self.inputs.shape == (self.n_init, self.get_n_parameters()), "inputs have not been initialized correctly"
        targets = np.atleast_1d(np.squeeze(np.array(targets)))
        assert targets.shape == (self.n_init,), "initial targets must have shape (n_init,)"
        self.targets = np.array(targets)
        self.initialized = True

    def run_initial_design(self):
        assert self.has_function(), "Design must have a bound function to use run_initial_design"
        inputs = self.generate_initial_design()
        targets = np.full((self.n_init,), np.nan)
        for i in range(self.n_init):
            targets[i] = np.array(self.f(inputs[i, :]))
        assert np.all(np.isfinite(targets)), "error in initializing sequential design, function outputs may not be the correct shape"
        self.set_initial_targets(targets)

    # -- one step -------------------------------------------------------------------------------------------
    def _generate_candidates(self):
        self.candidates = self.base_design.sample(self.n_cand)

    def _eval_metric(self):
        raise NotImplementedError("Base class for Sequential Design does not implement an evaluation metric")

    def _estimate_next_target(self, next_point):
        raise NotImplementedError("_estimate_next_point not implemented for base SequentialDesign")

    def _check_state(self, n_pending):
        """inputs hold `n_pending` points more than the targets, which cover `current_iteration` points."""
        if self.inputs is None:
            raise ValueError("Initial design has not been generated")
        assert self.inputs.shape == (self.current_iteration + n_pending, self.get_n_parameters()), "inputs have not been correctly updated"
        if self.targets is None:
            raise ValueError("Initial targets have not been generated")
        assert self.targets.shape == (self.current_iteration,), "targets have not been correctly updated"

    def get_next_point(self):
        """Draw fresh candidates, append the best one to the inputs and return it; its target is expected next."""
        self._check_state(0)
        self._generate_candidates()
        next_point = self.candidates[self._eval_metric(), :]
        self.inputs = np.vstack([self.inputs, next_point[None, :]])
        return next_point

    def set_next_target(self, target):
        self._check_state(1)
        target = np.atleast_1d(np.array(target))
        target = np.reshape(target, (len(target),))
        assert target.shape == (1,), "new target must have length 1"
        self.targets = np.append(self.targets, target.astype(np.float64))
        self.current_iteration += 1

    def get_batch_points(self, n_points):
        """n_points next points without running the simulator in between ("kriging believer"): after each point the design continues
        with the emulator's own prediction as its target.  Those stand-in targets are dropped again before returning, so the design
        then holds n_points inputs without targets: supply them with ``set_batch_targets``."""
        assert n_points > 0, "n_points must be positive"
        batch = np.zeros((n_points, self.get_n_parameters()))
        for i in range(n_points):
            batch[i] = self.get_next_point()
            self.set_next_target(self._estimate_next_target(batch[i]))
        self.current_iteration -= n_points
        self.targets = np.array(self.targets[:self.current_iteration])
        return batch

    def set_batch_targets(self, new_targets):
        if self.inputs is None:
            raise ValueError("Initial design has not been generated")
        n_points = self.inputs.shape[0] - self.current_iteration
        self._check_state(n_points)
        new_targets = np.atleast_1d(np.array(new_targets))
        new_targets = np.reshape(new_targets, (len(new_targets),))
        assert new_targets.shape == (n_points,), "new targets must have length n_points"
        self.targets = np.concatenate([self.targets, new_targets.astype(np.float64)])
        self.current_iteration += n_points

    # -- with a bound simulator -------------------------------------------------------------------------------
    def run_next_point(self):
        assert self.has_function(), "Design must have a bound function to use run_next_point"
        next_point = self.get_next_point()
        self.set_next_target(np.array(self.f(next_point)))

    def run_sequential_design(self, n_samples=None):
        assert self.has_function(), "Design must have a bound function to use run_sequential_design"
        if n_samples is None and self.n_samples is None:
            raise ValueError("must specify n_samples either when initializing or calling run_sequential_design")
        n_iter = self.n_samples if n_samples is None else n_samples
        assert n_iter >= 0, "number of samples must be non-negative"
        self.run_initial_design()
        for _ in range(n_iter):
            self.run_next_point()

    def __str__(self):
        lines = [type(self).__name__ + " with", self.get_base_design() + " base design"]
        if self.has_function():
            lines.append("a bound simulator function")
        lines += [str(self.get_n_samples()) + " total samples",
                  str(self.get_n_init()) + " initial points",
                  str(self.get_n_cand()) + " candidate points",
                  str(self.get_current_iteration()) + " current samples",
                  "current inputs: " + str(self.get_inputs()),
                  "current targets: " + str(self.get_targets())]
        return "\n".join(lines)


class MICEDesign(SequentialDesign):
    """MICE sequential design (Beck and Guillas 2016): the next point maximises the ratio of the emulator's predictive variance to the
    variance left at that point once all OTHER candidates are known (with the nugget scaled by ``nugget_s``).  ``nugget``: the base
    emulator's nugget, a string (``"adaptive"``, ``"fit"``) or a non-negative number.  The candidates' nugget is the base emulator's
    fitted value times ``nugget_s``: with ``"adaptive"`` that is the jitter the fit needed, which may be 0 -- many close candidates
    then cannot be factorised and the step fails after its attempts, as in the reference; give a number for large ``n_cand``."""

    N_FIT_ATTEMPTS = 10

    def __init__(self, base_design, f=None, n_samples=None, n_init=10, n_cand=50, nugget="adaptive", nugget_s=1.):
        if not isinstance(nugget, str):
            try:
                float(nugget)
            except TypeError:
                raise TypeError("nugget must be a string or convertible to a float")
            if nugget < 0.:
                raise ValueError("nugget parameter cannot be negative")
        if nugget_s < 0.:
            raise ValueError("nugget smoothing parameter cannot be negative")
        self.nugget = nugget if isinstance(nugget, str) else float(nugget)
        self.nugget_s = float(nugget_s)
        self.gp = None
        self._scores = None
        super().__init__(base_design, f, n_samples, n_init, n_cand)

    def get_nugget(self):
        return self.nugget

    def get_nugget_s(self):
        return self.nugget_s

    def _generate_candidates(self):
        super()._generate_candidates()
        self._scores = None                     # scores belong to one candidate set

    def _estimate_next_target(self, next_point):
        next_point = np.array(next_point)
        assert next_point.shape == (self.get_n_parameters(),), "bad shape for next_point"
        return self.gp.predict(next_point, unc=False, deriv=False)[0]

    def _score_candidates(self):
        """MICE criterion of every current candidate under the fitted ``self.gp``: one device factorisation for all of them."""
        self._scores, best = mice_criterion(self.gp, self.candidates, self.nugget_s)
        return best

    def _MICE_criterion(self, data_point):
        data_point = int(data_point)
        assert 0 <= data_point < self.n_cand, "test point index is out of range"
        if self._scores is None:
            self._score_candidates()
        return float(self._scores[data_point])

    # what a failed fit or factorisation says (fitting.py, the native "Unable to factorize matrix ..." / "All attempts at factorization
    # failed"): only these are worth another attempt from new random starting points
    _RETRY_ON = ("fitting failed", "did not converge", "factoriz")

    def _eval_metric(self):
        """Fit the emulator to the current design (up to N_FIT_ATTEMPTS tries: a fit starts from random points and can fail), score
        all candidates, return the index of the best.  Any other RuntimeError (no device, a shape the library refuses, a HIP error)
        is raised at once, unchanged."""
        if not LibGPGPU.gpu_usable():
            raise RuntimeError("Cannot run a MICEDesign step: the GPU library or a compatible GPU is unavailable")
        for attempt in range(self.N_FIT_ATTEMPTS):
            try:
                self.gp = fit_GP_MAP(GaussianProcessGPU(self.inputs, self.targets, nugget=self.nugget))
                return int(self._score_candidates())
            except RuntimeError as exc:
                if not any(key in str(exc) for key in self._RETRY_ON):
                    raise
                if attempt == self.N_FIT_ATTEMPTS - 1:
                    raise RuntimeError("Unable to find parameters suitable for both GPs") from exc


class ALCDesign(SequentialDesign):
    """ALC sequential design (active learning Cohn; Cohn 1996, Seo et al. 2000, Gramacy & Lee 2009): the next point is the candidate whose
    run reduces the emulator's predictive variance, averaged over ``n_ref`` fresh reference points drawn from the base design, the most
    (``ActiveLearning.alc_criterion``) -- equivalently the candidate that leaves the smallest integrated mean squared error.  Where
    ``MICEDesign`` scores a candidate by the variance at the candidate itself, this asks what the run does for the whole region.
    ``nugget``: the emulator's nugget as for ``MICEDesign``; ``noise``: the noise variance assumed for the new run (``None``: the
    emulator's nugget as its fit used it)."""

    N_FIT_ATTEMPTS = MICEDesign.N_FIT_ATTEMPTS
    _RETRY_ON = MICEDesign._RETRY_ON

    def __init__(self, base_design, f=None, n_samples=None, n_init=10, n_cand=50, n_ref=200, nugget="adaptive", noise=None):
        if not isinstance(nugget, str):
            try:
                float(nugget)
            except TypeError:
                raise TypeError("nugget must be a string or convertible to a float")
            if nugget < 0.:
                raise ValueError("nugget parameter cannot be negative")
        if int(n_ref) <= 0:
            raise ValueError("number of reference points must be positive")
        if noise is not None and not (float(noise) >= 0. and np.isfinite(float(noise))):
            raise ValueError("noise variance cannot be negative")
        self.nugget = nugget if isinstance(nugget, str) else float(nugget)
        self.n_ref = int(n_ref)
        self.noise = None if noise is None else float(noise)
        self.gp = None
        self.reference = None
        self._scores = None
        super().__init__(base_design, f, n_samples, n_init, n_cand)

    def get_nugget(self):
        return self.nugget

    def get_n_ref(self):
        return self.n_ref

    def get_noise(self):
        return self.noise

    def save_design(self, filename):
        """inputs, targets and candidates as the base class stores them, with n_ref and noise."""
        np.savez(filename, inputs=self.inputs, targets=self.targets, candidates=self.candidates, n_ref=self.n_ref, noise=self.noise)

    def load_design(self, filename):
        super().load_design(filename)
        with np.load(filename, allow_pickle=True) as archive:
            if "n_ref" in archive.files:
                self.n_ref = int(archive["n_ref"])
                noise = _none_or_array(archive["noise"])
                self.noise = None if noise is None else float(noise)

    def _generate_candidates(self):
        super()._generate_candidates()
        self._scores = None                     # scores belong to one candidate set

    def _estimate_next_target(self, next_point):
        next_point = np.array(next_point)
        assert next_point.shape == (self.get_n_parameters(),), "bad shape for next_point"
        return self.gp.predict(next_point, unc=False, deriv=False)[0]

    def _score_candidates(self):
        """ALC of every current candidate under the fitted ``self.gp`` over fresh reference points: one device call."""
        from .ActiveLearning import alc_criterion
        self.reference = self.base_design.sample(self.n_ref)
        res = alc_criterion(self.gp, self.candidates, self.reference, noise=self.noise)
        self._scores = res.reduction[0]
        return int(res.best[0])

    def _eval_metric(self):
        """Fit the emulator to the current design (up to N_FIT_ATTEMPTS tries, as ``MICEDesign._eval_metric``), score all candidates,
        return the index of the best."""
        if not LibGPGPU.gpu_usable():
            raise RuntimeError("Cannot run an ALCDesign step: the GPU library or a compatible GPU is unavailable")
        for attempt in range(self.N_FIT_ATTEMPTS):
            try:
                self.gp = fit_GP_MAP(GaussianProcessGPU(self.inputs, self.targets, nugget=self.nugget))
                return int(self._score_candidates())
            except RuntimeError as exc:
                if not any(key in str(exc) for key in self._RETRY_ON):
                    raise
                if attempt == self.N_FIT_ATTEMPTS - 1:
                    raise RuntimeError("Unable to find parameters suitable for the emulator") from exc

    def _fit_emulator(self):
        """``self.gp`` fitted to the current design, with the retries of ``_eval_metric``."""
        if not LibGPGPU.gpu_usable():
            raise RuntimeError("Cannot run an ALCDesign step: the GPU library or a compatible GPU is unavailable")
        for attempt in range(self.N_FIT_ATTEMPTS):
            try:
                self.gp = fit_GP_MAP(GaussianProcessGPU(self.inputs, self.targets, nugget=self.nugget))
                return
            except RuntimeError as exc:
                if not any(key in str(exc) for key in self._RETRY_ON):
                    raise
                if attempt == self.N_FIT_ATTEMPTS - 1:
                    raise RuntimeError("Unable to find parameters suitable for the emulator") from exc

    def get_conditioned_batch(self, n_points):
        """n_points next points from ONE fit, one candidate set, one reference set and one ``ActiveLearning.alc_batch`` call: after each
        pick the emulator's posterior is conditioned on a run there, on the device, at the fitted hyperparameters -- the variance does
        not depend on the target, so no stand-in target and no refit are needed (``get_batch_points``, the kriging believer, refits
        n_points times).  The design then holds the batch as inputs without targets, as ``get_batch_points`` leaves it: supply them with
        ``set_batch_targets``.  Fewer than n_points rows come back where the criterion has nothing left to gain
        (``ALCBatchResult.n_picked``); the result of the call is kept in ``self.batch_result``."""
        from .ActiveLearning import alc_batch
        n_points = int(n_points)
        assert n_points > 0, "n_points must be positive"
        self._check_state(0)
        self._generate_candidates()
        self._fit_emulator()
        self.reference = self.base_design.sample(self.n_ref)
        self.batch_result = alc_batch(self.gp, self.candidates, self.reference, n_points, noise=self.noise, keep_scores=False)
        batch = np.array(self.batch_result.points[0][:int(self.batch_result.n_picked[0])])
        self.inputs = np.vstack([self.inputs, batch])
        return batch
