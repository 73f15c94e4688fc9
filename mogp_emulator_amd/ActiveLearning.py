"""
Active learning with a fitted emulator: the posterior covariance between two point sets and the ALC design criterion built on it.

At fixed hyperparameters, with Q = K + nugget I = L L^T as the fit left it and v(x) = L^-1 k(x),

    c(x, x') = sigma^2 k(x, x') - v(x)^T v(x')          posterior covariance of the latent function (``predict_cov``)
    s^2(x)   = max(c(x, x), 0)                          what ``predict(..., include_nugget=False)`` returns as ``unc``

One more run at c with noise variance tau >= 0 reduces the variance at r by c(r, c)^2 / (s^2(c) + tau), and the ALC criterion (active
learning Cohn: Cohn 1996, Seo et al. 2000, Gramacy & Lee 2009; equivalently the IMSE reduction) is that reduction summed over reference
points r_1 .. r_m with weights w_j >= 0 (default 1 / m):

    ALC(c) = sum_j w_j c(r_j, c)^2 / (s^2(c) + tau),     integrated variance after the run = sum_j w_j s^2(r_j) - ALC(c).

The best candidate by ALC is the best by IMSE.  On the device V = L^-1 K*^T of either point set is what ``predict(full_cov=True)``
stores, V_c^T V_r is an fp64-MFMA product, and for ALC the (m_c, m_r) matrix never exists: it is squared, weighted and summed along the
reference points in the product's epilogue (``csrc/kernels_alc.hip``); m_c numbers per emulator come back.  Both variances come from the
predictive-variance launches of ``predict`` itself, so the criterion is consistent with what ``predict`` shows, bit for bit.

Floor: a candidate whose s^2(c) + tau is at or below (n + 2) 2^-52 sigma^2 -- the rounding of sigma^2 minus a sum of n squares -- has no
meaningful ratio (a candidate on a training point of an emulator with no nugget): it gets ALC 0 and ``degenerate`` True.  No NaN, no
exception.

Not covered: ``nugget="pivot"`` and ``analytic_mean=True`` (``RuntimeError``; the covariance gains a rank-q term there),
``dist.ShardedMultiOutputGP``, and ALC averaged over hyperparameter samples.

Batches (``alc_batch``): at fixed hyperparameters the predictive variance does not depend on the targets, so the posterior can be
conditioned on a pick before its run has come back.  A run at p with noise tau appends one row to the Cholesky factor, which gives every
stored v(x) one more entry

    u(x) = c(x, p) / sqrt(s^2(p) + tau),     c_new(x, x') = c(x, x') - u(x) u(x'),     s^2_new(x) = s^2(x) - u(x)^2,

and after t picks the ALC of every remaining candidate is the same product over n + t rows.  V of both point sets is built once per call;
a pick costs no n^3 and no (m_c + m_r) n^2 work, and in ``select="each"`` the picks of a batch are enqueued back to back without the host
in between.  Points already submitted (``pending``) are conditioned on first.  Not covered for batches: replicate picks (a picked
candidate is masked) and the O(m_c m_r D)-per-pick downdate of the numerators, which would trade this exact route for cancellation.
"""
import numpy as np


class ALCResult(object):
    """What ``alc_criterion`` returns (E = 1 for a ``GaussianProcessGPU``):

    * ``reduction`` (E, m_c)       ALC of every candidate; NaN rows for emulators that are not fit
    * ``cand_variance`` (E, m_c)   s^2 at the candidates, ``predict(candidates, include_nugget=False).unc`` bit for bit
    * ``ref_variance`` (E, m_r)    s^2 at the reference points, likewise
    * ``degenerate`` (E, m_c)      True where s^2(c) + noise is at or below the floor (``reduction`` is 0 there)
    * ``noise`` (E,)               the noise variance tau used
    * ``weights`` (m_r,)           the weights used"""

    def __init__(self, reduction, cand_variance, ref_variance, degenerate, noise, weights):
        self.reduction, self.cand_variance, self.ref_variance = reduction, cand_variance, ref_variance
        self.degenerate, self.noise, self.weights = degenerate, noise, weights

    @property
    def integrated_variance(self):
        """(E,) the weighted predictive variance over the reference points before the run"""
        return self.ref_variance @ self.weights

    @property
    def best(self):
        """(E,) index of the best candidate per emulator (0 for an emulator that is not fit)"""
        red = np.where(np.isnan(self.reduction), -np.inf, self.reduction)
        return np.argmax(red, axis=1)

    def total(self, scale=True):
        """(m_c,) the sum over the fitted emulators of ``reduction / integrated_variance[:, None]`` (``scale=False``: of ``reduction``):
        one score per candidate for choosing one point for a multi-output model."""
        fitted = ~np.any(np.isnan(self.reduction), axis=1)
        red = self.reduction[fitted]
        if scale:
            red = red / self.integrated_variance[fitted][:, None]
        return red.sum(axis=0)


def _points(name, who, x, D):
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1) if D == 1 else x.reshape(1, -1)
    if x.ndim != 2 or x.shape[1] != D or x.shape[0] < 1:
        raise ValueError("%s: %s must have shape (m, D) with D = %d and at least one point" % (who, name, D))
    if not np.all(np.isfinite(x)):
        raise ValueError("%s: %s must be finite" % (who, name))
    return x


def _native(who, gp, max_a, max_b):
    """the checks that need no device, then (native handle, single)"""
    from . import LibGPGPU
    if not LibGPGPU.HAVE_LIBGPGPU:
        raise TypeError("%s needs a GaussianProcessGPU or a MultiOutputGP_GPU (the device library is not loaded)" % who)
    from .GaussianProcessGPU import GaussianProcessGPU
    from .MultiOutputGP_GPU import MultiOutputGP_GPU
    if not isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)):
        raise TypeError("%s needs a GaussianProcessGPU or a MultiOutputGP_GPU" % who)
    single = isinstance(gp, GaussianProcessGPU)
    if int(max_a) < 0 or int(max_b) < 0:
        raise ValueError("%s: max_slots and max_points must not be negative" % who)
    return single


def _fit_state(who, gp, single):
    pivot = gp.nugget_type == "pivot" if single else gp._nugget_name == "pivot"
    if pivot:
        raise RuntimeError("%s: not available with nugget=\"pivot\"" % who)
    if getattr(gp, "_analytic_mean", False):
        raise RuntimeError("%s: not available with analytic_mean=True" % who)
    native = gp._densegp_gpu if single else gp._mogp_gpu
    if single and not native.theta_fit_status():
        raise RuntimeError("%s: hyperparameters have not been fit for this Gaussian Process" % who)
    return native


def _alc_args(who, gp, candidates, reference, weights, noise):
    """what alc_criterion and alc_batch check alike, before the device: (candidates, reference, weights, noise) as arrays / float"""
    D = int(gp.D)
    candidates = _points("candidates", who, candidates, D)
    reference = _points("reference", who, reference, D)
    mr = reference.shape[0]
    if weights is None:
        weights = np.full(mr, 1. / mr)
    else:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (mr,):
            raise ValueError("%s: weights must have shape (m_r,) with m_r = %d" % (who, mr))
        if not np.all(np.isfinite(weights)):
            raise ValueError("%s: weights must be finite" % who)
        if np.any(weights < 0.):
            raise ValueError("%s: weights must not be negative" % who)
        if not weights.sum() > 0.:
            raise ValueError("%s: weights must not sum to 0" % who)
    if noise is not None:
        noise = float(noise)
        if not (noise >= 0. and np.isfinite(noise)):
            raise ValueError("%s: noise must be a finite number that is not negative" % who)
    return candidates, reference, weights, noise


def predict_cov(gp, X1, X2=None, max_slots=0):
    """The posterior covariance c(X1, X2) of the latent function per emulator of a fitted ``GaussianProcessGPU`` (E = 1) or
    ``MultiOutputGP_GPU`` (the multi-device form included), computed on the device: an ``ndarray`` (E, m1, m2), nugget not included.
    ``X2=None`` means X2 = X1.  It is the off-diagonal block of ``predict(full_cov=True)`` on the stacked points without the two diagonal
    blocks.  Refused above the 64 GB scratch rule of ``full_cov`` (V of both sets, the output and the cross-covariance scratch counted).
    ``max_slots`` caps the emulators per group (0: the library's choice).

    Every argument is checked before the device is touched.  ``RuntimeError`` for ``nugget="pivot"``, ``analytic_mean=True`` and a
    ``GaussianProcessGPU`` that is not fit; emulators of a ``MultiOutputGP_GPU`` that are not fit give NaN rows."""
    who = "predict_cov"
    single = _native(who, gp, max_slots, 0)
    D = int(gp.D)
    X1 = _points("X1", who, X1, D)
    X2 = None if X2 is None else _points("X2", who, X2, D)
    native = _fit_state(who, gp, single)
    cov = native.predict_cov(X1, X2, max_slots=int(max_slots))
    return cov[None] if single else cov


def alc_criterion(gp, candidates, reference, weights=None, noise=None, max_slots=0, max_points=0):
    """The ALC criterion of ``candidates`` (m_c, D) over the reference points ``reference`` (m_r, D) for a fitted ``GaussianProcessGPU``
    (E = 1) or ``MultiOutputGP_GPU`` (the multi-device form included), computed on the device; see the module docstring for the formulas.

    ``weights`` (m_r,) >= 0, default 1 / m_r.  ``noise``: the noise variance of the new run, ``None`` for each emulator's nugget as its
    fit used it, or a float >= 0 for all emulators.  ``max_points`` caps the reference points per chunk (rounded down to a multiple of
    128), ``max_slots`` the emulators per group; 0 is the library's choice, and neither changes a bit of the result.

    Every argument is checked before the device is touched.  ``RuntimeError`` for ``nugget="pivot"``, ``analytic_mean=True`` and a
    ``GaussianProcessGPU`` that is not fit; emulators of a ``MultiOutputGP_GPU`` that are not fit give NaN rows.  Returns an ``ALCResult``."""
    who = "alc_criterion"
    single = _native(who, gp, max_slots, max_points)
    candidates, reference, weights, noise = _alc_args(who, gp, candidates, reference, weights, noise)
    native = _fit_state(who, gp, single)
    if single:
        tau = np.array([float(gp.nugget) if noise is None else noise])
        red, cv, rv, deg = native.alc(candidates, reference, weights, noise=tau[0], max_slots=int(max_slots), max_points=int(max_points))
        red, cv, rv, deg = red[None], cv[None], rv[None], deg[None]
    else:
        tau = np.asarray(gp._nuggets(), dtype=np.float64) if noise is None else np.full(int(gp.n_emulators), noise)
        red, cv, rv, deg = native.alc(candidates, reference, weights, noise=np.ascontiguousarray(tau), max_slots=int(max_slots),
                                      max_points=int(max_points))
    return ALCResult(reduction=red, cand_variance=cv, ref_variance=rv, degenerate=deg, noise=tau, weights=weights)


class ALCBatchResult(object):
    """What ``alc_batch`` returns (E = 1 for a ``GaussianProcessGPU``; q = ``n_points``):

    * ``picks``                    ``select="each"``: (E, q) candidate indices, every emulator its own batch; ``select="total"``: (q,),
                                   one batch for the model.  -1 beyond ``n_picked`` (and in rows of emulators that are not fit)
    * ``n_picked`` (E,)            picks made before the stopping rule ended the batch; with ``select="total"`` the steps in which that
                                   emulator was conditioned on the model's pick
    * ``emulator_picks`` (E, q)    what each emulator was conditioned on (``picks`` itself with ``select="each"``)
    * ``points``                   the picked rows of ``candidates``, shaped like ``picks`` + (D,); NaN where the pick is -1
    * ``pick_reduction`` (E, q)    the ALC of each emulator's pick at its step (0 where there is none)
    * ``reduction`` (E, q, m_c)    with ``keep_scores``: the ALC of every candidate at every step, else None
    * ``degenerate`` (E, q, m_c)   with ``keep_scores``: the floor rule at every step, else None
    * ``cand_variance`` (E, m_c), ``ref_variance`` (E, m_r)   s^2 before any pick (pending points included): ``predict``'s own bits
    * ``ref_variance_after`` (E, m_r)    s^2 at the reference points after the last pick
    * ``integrated_variance`` (E, q + 1) IV_0 after the pending points, IV_t = IV_{t-1} - reduction_t[pick_t]
    * ``pending_skipped`` (E,)     pending points that failed the floor test and were not conditioned on
    * ``noise`` (E,), ``weights`` (m_r,)"""

    def __init__(self, picks, emulator_picks, points, pick_reduction, reduction, degenerate, cand_variance, ref_variance, ref_variance_after,
                 integrated_variance, pending_skipped, noise, weights):
        self.picks, self.emulator_picks, self.points, self.pick_reduction = picks, emulator_picks, points, pick_reduction
        self.reduction, self.degenerate, self.cand_variance, self.ref_variance = reduction, degenerate, cand_variance, ref_variance
        self.ref_variance_after, self.integrated_variance, self.pending_skipped = ref_variance_after, integrated_variance, pending_skipped
        self.noise, self.weights = noise, weights

    @property
    def n_picked(self):
        return np.sum(self.emulator_picks >= 0, axis=1)

    @property
    def total_reduction(self):
        """(E,) what the whole batch takes off the integrated variance: IV_0 - IV_q"""
        return self.integrated_variance[:, 0] - self.integrated_variance[:, -1]


def alc_batch(gp, candidates, reference, n_points, weights=None, noise=None, pending=None, select="each", keep_scores=True, max_slots=0):
    """A greedy batch of ``n_points`` ALC picks from ``candidates`` (m_c, D) over the reference points ``reference`` (m_r, D) for a fitted
    ``GaussianProcessGPU`` (E = 1) or ``MultiOutputGP_GPU`` (the multi-device form included): after each pick the posterior is conditioned
    on a run there with noise variance tau -- on the device, at the fitted hyperparameters, without a target -- and the next pick is
    scored under it.  See the module docstring for the formulas.

    ``weights`` and ``noise`` as in ``alc_criterion``.  ``pending`` (P, D): points already submitted whose results are not back; the
    posterior is conditioned on them first, in order, with the same tau.  ``select="each"``: every emulator its own batch;
    ``select="total"``: one batch for the model, each step the candidate with the largest sum over the fitted emulators of
    ``reduction_e / IV_e`` (IV_e the integrated variance before that step): ``ALCResult.total(scale=True)`` of the conditioned model.
    Arg-max ties go to the lowest index, a picked candidate is never picked again, and a batch stops -- picks of -1, nothing NaN, nothing
    raised -- when the best remaining score is 0 or its denominator is at or below the floor (n + t + 2) 2^-52 sigma^2.
    ``keep_scores=False`` skips the download of every step's scores.  ``max_slots`` caps the emulators per group in ``select="each"``
    (0: the library's choice) and changes no bit; ``select="total"`` needs all fitted emulators of a device in one group.

    Every argument is checked before the device is touched; refused: what ``alc_criterion`` refuses, ``n_points < 1``,
    ``n_points > m_c`` and an unknown ``select``.  Emulators of a ``MultiOutputGP_GPU`` that are not fit give NaN rows and picks of -1 and
    are left out of ``select="total"``.  Returns an ``ALCBatchResult``."""
    who = "alc_batch"
    single = _native(who, gp, max_slots, 0)
    if select not in ("each", "total"):
        raise ValueError("%s: select must be \"each\" or \"total\"" % who)
    candidates, reference, weights, noise = _alc_args(who, gp, candidates, reference, weights, noise)
    q, mc, D = int(n_points), candidates.shape[0], int(gp.D)
    if q < 1:
        raise ValueError("%s: n_points must be at least 1" % who)
    if q > mc:
        raise ValueError("%s: n_points must not exceed the number of candidates (%d)" % (who, mc))
    P = 0
    x = candidates
    if pending is not None:
        pending = _points("pending", who, pending, D)
        P = pending.shape[0]
        x = np.ascontiguousarray(np.vstack([pending, candidates]))
    native = _fit_state(who, gp, single)
    if single:
        tau = np.array([float(gp.nugget) if noise is None else noise])
        r = native.alc_batch(x, P, reference, weights, q, noise=tau[0], max_slots=int(max_slots), keep_scores=bool(keep_scores))
        r = {k: (v if v is None or k == "total_picks" else v[None]) for k, v in r.items()}
        if select == "total":
            r["total_picks"] = r["picks"][0]
    else:
        tau = np.asarray(gp._nuggets(), dtype=np.float64) if noise is None else np.full(int(gp.n_emulators), noise)
        r = native.alc_batch(x, P, reference, weights, q, noise=np.ascontiguousarray(tau), total=select == "total", max_slots=int(max_slots),
                             keep_scores=bool(keep_scores))

    def index(p):                       # candidate numbers without the pending prefix
        return np.where(p >= 0, p - P, -1).astype(np.int64)
    own = index(r["picks"][:, P:])
    picks = own if select == "each" else index(r["total_picks"][P:])
    points = np.where((picks >= 0)[..., None], candidates[np.maximum(picks, 0)], np.nan)
    fitted = ~np.isnan(r["iv"][:, 0])
    return ALCBatchResult(picks=picks, emulator_picks=own, points=points, pick_reduction=r["pick_red"][:, P:],
                          reduction=None if r["red"] is None else r["red"][:, P:, P:],
                          degenerate=None if r["deg"] is None else r["deg"][:, P:, P:],
                          cand_variance=r["cand_var"][:, P:], ref_variance=r["ref_var"], ref_variance_after=r["ref_var_after"],
                          integrated_variance=r["iv"][:, P:], pending_skipped=np.where(fitted, np.sum(r["picks"][:, :P] < 0, axis=1), 0),
                          noise=tau, weights=weights)
