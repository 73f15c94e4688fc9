"""
Predictions averaged over the hyperparameter posterior instead of plugged in at the MAP point.

With samples theta_s and normalised weights w_s, mu_s / v_s the predictive mean / variance of the emulator at theta_s,

    mean    = sum w_s mu_s
    within  = sum w_s v_s                       (the average predictive variance)
    between = sum w_s (mu_s - mean)^2           (how far the samples disagree about the mean)
    unc     = within + between                  (law of total variance)

Every sample is factored on the device in one batched pass beside the fitted emulator (the replica engine of ``fit_GP_MAP``), all of them
are predicted at once and reduced over the samples on the device (``csrc/kernels_mixture.hip``): three numbers per query point come back,
and the emulator keeps its MAP fit.  The samples come from the Laplace approximation N(theta_hat, H^-1) (``Laplace.py``) -- uniform
weights, or with ``importance=True`` self-normalised importance weights against the true posterior -- or are the caller's own (MCMC draws).

Not covered (``RuntimeError``): ``nugget="pivot"`` and ``analytic_mean=True``.
"""
import numpy as np

from .Laplace import laplace_approximation, _theta_of

# log proposal density of a sample that must get weight exactly 0 (exp(-1e300) == 0): the padding samples of an emulator whose Hessian is
# not positive definite
_LOG_Q_NEVER = 1e300


def effective_sample_size(weights):
    """1 / sum w^2 over the last axis of normalised weights (NaN where they are)"""
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1. / np.sum(w * w, axis=-1)


def mixture_weights(logpost, ok, log_q=None, weights=None):
    """Normalised weights and effective sample size of S samples (last axis; any leading axes) from their negative log-posteriors
    ``logpost`` (F), their ``ok`` flags and EITHER the log proposal density ``log_q`` (up to a constant) OR explicit ``weights``:

        log_q:    l_s = -(F_s - F_a) - (log_q_s - log_q_a),  a = the first ok sample with the smallest F,   w_s = exp(l_s - max l)
        weights:  w_s = weights_s

    Samples that are not ok get weight 0, then the weights are divided by their sum.  No ok sample, or a sum that is not a positive
    finite number: NaN weights and NaN ess.  Returns (w, ess) with ess = 1 / sum w^2.  This is the formula the device call applies
    (``mixture_weights`` in ``csrc/predict_plan.h``)."""
    if (log_q is None) == (weights is None):
        raise ValueError("exactly one of log_q and weights must be given")
    F = np.asarray(logpost, dtype=np.float64)
    ok = np.asarray(ok, dtype=bool)
    if ok.shape != F.shape:
        raise ValueError("logpost and ok must have the same shape")
    src = np.asarray(log_q if weights is None else weights, dtype=np.float64)
    if src.shape != F.shape:
        raise ValueError("log_q / weights must have the shape of logpost")
    lead = F.shape[:-1]
    S = F.shape[-1]
    F2, ok2, src2 = F.reshape(-1, S), ok.reshape(-1, S), src.reshape(-1, S)
    w = np.full(F2.shape, np.nan)
    for r in range(F2.shape[0]):
        good = np.flatnonzero(ok2[r])
        if good.size == 0:
            continue
        if weights is None:
            a = good[np.argmin(F2[r, good])]                   # argmin returns the first of equal minima
            l = -(F2[r, good] - F2[r, a]) - (src2[r, good] - src2[r, a])
            v = np.zeros(S)
            v[good] = np.exp(l - l.max())
        else:
            v = np.where(ok2[r], src2[r], 0.)
        tot = 0.
        for x in v:                                             # the device's host code sums in sample order
            tot += x
        if tot > 0. and np.isfinite(tot):
            w[r] = v / tot
    w = w.reshape(lead + (S,))
    return w, effective_sample_size(w)


class MarginalPredictResult(object):
    """``mean``, ``unc`` (= ``within`` + ``between``), ``within``, ``between`` per query point; ``weights`` (normalised), ``thetas``,
    ``logpost`` (negative log-posterior F, NaN where the sample failed) and ``ok`` per sample; ``ess`` = 1 / sum w^2; ``laplace_ok``:
    the samples came from a Laplace approximation whose Hessian is positive definite (None with the caller's own samples).
    ``GaussianProcessGPU``: (m,) and (S,) arrays; ``MultiOutputGP_GPU``: (n_emulators, m) and (n_emulators, S)."""

    _fields = ("mean", "unc", "within", "between", "weights", "thetas", "logpost", "ok", "ess", "laplace_ok")

    def __init__(self, **kw):
        for f in self._fields:
            setattr(self, f, kw[f])

    def __repr__(self):
        return "MarginalPredictResult(mean=%s, unc=%s, ess=%s, laplace_ok=%s)" % (self.mean, self.unc, self.ess, self.laplace_ok)


def _check_samples(thetas, weights, lead, width):
    """the caller's own samples: thetas ``lead + (S, width)`` finite, weights ``lead + (S,)`` finite and non-negative (None: uniform)"""
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    if th.ndim != len(lead) + 2 or th.shape[:len(lead)] != tuple(lead) or th.shape[-1] != width or th.shape[-2] < 1:
        raise ValueError("thetas must have shape %s with S >= 1" % (tuple(lead) + ("S", width),))
    if not np.all(np.isfinite(th)):
        raise ValueError("thetas must be finite")
    if weights is None:
        w = np.ones(th.shape[:-1])
    else:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != th.shape[:-1]:
            raise ValueError("weights must have shape %s" % (th.shape[:-1],))
        if not np.all(np.isfinite(w)):
            raise ValueError("weights must be finite")
        if np.any(w < 0.):
            raise ValueError("weights must not be negative")
    return th, w


def predict_marginal(gp, testing, thetas=None, weights=None, n_samples=32, rng=None, importance=True, include_nugget=True,
                     max_slots=0, max_points=0):
    """Prediction of a fitted ``GaussianProcessGPU`` or ``MultiOutputGP_GPU`` at ``testing`` (m, D), averaged over hyperparameter samples.

    ``thetas=None``: ``n_samples`` draws per emulator from ``laplace_approximation(gp)`` (one ``rng`` -- Generator, seed or None --,
    emulators in index order); ``importance=True`` weights them by posterior / proposal (self-normalised importance sampling, proposal
    density from ``LaplaceResult.logpdf``), ``importance=False`` uniformly.  Where the Hessian at the fitted theta is not positive definite
    a single GP raises ``ValueError``; an emulator of a multi-output model is predicted at its fitted theta alone (sample 0 = theta_hat
    with weight 1, the others weight 0) and has ``laplace_ok`` False.
    ``thetas`` given ((S, P), or (n_emulators, S, P)): the caller's samples with ``weights`` ((S,) / (n_emulators, S); None: uniform).

    ``max_slots`` / ``max_points`` bound the samples factored per pass and the query points per chunk (0: the library's choice); the
    result does not depend on them, bit for bit.  Returns a ``MarginalPredictResult``."""
    if thetas is None and weights is not None:
        raise ValueError("weights need thetas: the weights of Laplace draws are computed, not given")
    if thetas is None and int(n_samples) < 1:
        raise ValueError("n_samples must be at least 1")
    if int(max_slots) < 0 or int(max_points) < 0:
        raise ValueError("max_slots and max_points must not be negative")
    from . import LibGPGPU
    if not LibGPGPU.HAVE_LIBGPGPU:
        raise TypeError("predict_marginal needs a GaussianProcessGPU or a MultiOutputGP_GPU (the device library is not loaded)")
    from .GaussianProcessGPU import GaussianProcessGPU
    from .MultiOutputGP_GPU import MultiOutputGP_GPU
    if not isinstance(gp, (GaussianProcessGPU, MultiOutputGP_GPU)):
        raise TypeError("predict_marginal needs a GaussianProcessGPU or a MultiOutputGP_GPU")
    testing = np.ascontiguousarray(testing, dtype=np.float64)
    if testing.ndim == 1:
        testing = testing.reshape(-1, 1) if gp.D == 1 else testing.reshape(1, -1)
    if testing.ndim != 2 or testing.shape[1] != gp.D:
        raise ValueError("testing must have shape (m, D)")
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    S = int(n_samples)

    if isinstance(gp, GaussianProcessGPU):
        if _theta_of(gp._densegp_gpu) is None:
            raise ValueError("hyperparameters have not been fit for this Gaussian Process")
        log_q, laplace_ok = None, None
        if thetas is None:
            lap = laplace_approximation(gp)
            th = np.ascontiguousarray(lap.sample(S, rng))                # ValueError where the Hessian is not positive definite
            laplace_ok = True
            if importance:
                log_q, w = lap.logpdf(th), None
            else:
                w = np.ones(S)
        else:
            th, w = _check_samples(thetas, weights, (), gp.n_params)
        mean, within, between, wout, lp, ok = gp._densegp_gpu.predict_mixture(th, testing, weights=w, log_q=log_q,
                                                                              include_nugget=include_nugget, max_slots=max_slots,
                                                                              max_points=max_points)
        return MarginalPredictResult(mean=mean, unc=within + between, within=within, between=between, weights=wout, thetas=th,
                                     logpost=lp, ok=ok, ess=float(effective_sample_size(wout)), laplace_ok=laplace_ok)

    ne = gp.n_emulators
    widths = [gp._mogp_gpu.emulator(i).n_params() for i in range(ne)]
    width = max(widths)
    log_q, laplace_ok = None, None
    if thetas is None:
        laps = laplace_approximation(gp)
        th = np.zeros((ne, S, width))
        log_q = np.zeros((ne, S))
        w = np.ones((ne, S))
        laplace_ok = np.zeros(ne, dtype=bool)
        for i, lap in enumerate(laps):
            if lap is None:                                               # not fit: a NaN row comes back
                continue
            P = widths[i]
            if lap.is_minimum:
                th[i, :, :P] = lap.sample(S, rng)
                laplace_ok[i] = True
                log_q[i] = lap.logpdf(th[i, :, :P])
            else:                                                         # the plug-in prediction: theta_hat with weight 1
                th[i, :, :P] = lap.theta
                log_q[i, 1:] = _LOG_Q_NEVER
                w[i, 1:] = 0.
        if importance:
            w = None
        else:
            log_q = None
    else:
        th, w = _check_samples(thetas, weights, (ne,), width)
    mean, within, between, wout, lp, ok, _ = gp._mogp_gpu.predict_mixture(th, testing, weights=w, log_q=log_q, include_nugget=include_nugget,
                                                                         max_slots=max_slots, max_points=max_points)
    return MarginalPredictResult(mean=mean, unc=within + between, within=within, between=between, weights=wout, thetas=th, logpost=lp,
                                 ok=ok, ess=effective_sample_size(wout), laplace_ok=laplace_ok)
