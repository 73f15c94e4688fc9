"""
Generate tests/golden/gkdr.npz by IMPORTING THE REAL REFERENCE (mogp_emulator.DimensionReduction), as make_golden.py does.

Runs only in the build container, never from the tests, with the reference package importable (see make_golden.py for the
environment):

    PYTHONPATH=<reference package> python -W ignore tests/golden/make_golden_gkdr.py

The outputs are data only: inputs and the reference's outputs on them.  R is the matrix the reference hands to
np.linalg.eigh (captured there), B its sorted eigenvectors; the tuning sequence is what the reference's tune_parameters
evaluates with a deterministic train_model (least squares with an intercept on the reduced inputs).
"""
import os
import sys

import numpy as np

import mogp_emulator
from mogp_emulator import DimensionReduction as DR
from mogp_emulator.DimensionReduction import gKDR, gram_matrix, gram_matrix_sqexp, median_dist

HERE = os.path.dirname(os.path.abspath(__file__))


def lstsq_model(X, Y):
    A = np.hstack([np.ones((X.shape[0], 1)), X])
    coef = np.linalg.lstsq(A, Y, rcond=None)[0]
    return lambda Z: np.hstack([np.ones((Z.shape[0], 1)), Z]) @ coef


def run(X, Y, **kw):
    """(R, B) of the reference gKDR: R captured at its np.linalg.eigh call."""
    seen = []
    eigh = np.linalg.eigh

    def capture(R):
        seen.append(np.array(R, dtype=np.float64, copy=True))
        return eigh(R)
    np.linalg.eigh = capture
    try:
        dr = gKDR(X, Y, **kw)
    finally:
        np.linalg.eigh = eigh
    assert len(seen) == 1
    return seen[0], dr.B


def target(X, rng):
    return np.sin(2 * X[:, 0] + X[:, 1]) + 0.5 * X[:, 2] ** 2 + 0.01 * rng.normal(size=X.shape[0])


out = {}
rng = np.random.default_rng(2024)

# host helpers
H = rng.normal(size=(17, 3))
out["h_X"] = H
out["h_median"] = np.array(median_dist(H))
out["h_median_y"] = np.array(median_dist(H[:, :1]))
out["h_sqexp"] = gram_matrix_sqexp(H, 0.7)
out["h_dot"] = gram_matrix(H, lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2])

# R / B cases: (name, N, M, offset, keyword arguments)
cases = [("n200", 200, 5, 0.0, {}),
         ("n300_off", 300, 8, 1000.0, {"X_scale": 0.5, "Y_scale": 2.0}),
         ("sg", 150, 4, 0.0, {"SGX": 0.7, "SGY": 0.3}),
         ("eps0", 100, 3, 0.0, {"EPS": 0.0, "X_scale": 0.2}),
         ("n1000", 1000, 10, 0.0, {}),
         ("n2000", 2000, 10, 0.0, {})]
names = []
for name, N, M, off, kw in cases:
    X = rng.uniform(0, 1, (N, M))
    Y = target(X, rng)
    X = X + off
    R, B = run(X, Y, **kw)
    names.append(name)
    out[name + "_X"] = X
    out[name + "_Y"] = Y
    out[name + "_R"] = R
    out[name + "_B"] = B
    for k in ["X_scale", "Y_scale", "EPS", "SGX", "SGY"]:
        out[name + "_" + k] = np.array(np.nan if kw.get(k) is None else kw[k])
    print(name, "done", flush=True)
out["cases"] = np.array(names)

# EPS = 0 with rows 0 and 1 equal: the second pivot of Kx is exactly 0 and cho_factor raises
Xd = rng.uniform(0, 1, (40, 3))
Xd[1] = Xd[0]
Yd = target(Xd, rng)
try:
    gKDR(Xd, Yd, EPS=0.0)
    raise AssertionError("the reference accepted a singular Kx")
except np.linalg.LinAlgError:
    pass
out["dup_X"], out["dup_Y"] = Xd, Yd

# tune_parameters with a deterministic train_model: the sequence of (K, cX, cY, loss) the search evaluates
Xt = rng.uniform(0, 1, (120, 6))
Yt = target(Xt, rng)
seq = []
loss_fn = gKDR._compute_loss


def recording(X, Y, train_model, folds, *params, **kw):
    loss = loss_fn(X, Y, train_model, folds, *params, **kw)
    seq.append(tuple(params) + (loss,))
    return loss
gKDR._compute_loss = staticmethod(recording)
try:
    dr, tune_loss = gKDR.tune_parameters(Xt, Yt, lstsq_model, maxK=4)
finally:
    gKDR._compute_loss = staticmethod(loss_fn)
seq = np.array(seq, dtype=np.float64)
# every comparison the search makes (consecutive K of one (cX, cY), each run's result against the running minimum) must be
# decided by more than 1e-3 relative, so that rounding cannot flip it
def apart(a, b):
    assert abs(a - b) > 1e-3 * max(abs(a), abs(b)), (a, b)
best = np.inf
runs = {}
for k, cX, cY, l in seq:
    runs.setdefault((cX, cY), []).append((k, l))
for run in runs.values():
    for (_, a), (_, b) in zip(run, run[1:]):
        apart(a, b)
    cand = run[-2][1] if len(run) > 1 and run[-2][1] < run[-1][1] else run[-1][1]
    if np.isfinite(best):
        apart(cand, best)
    best = min(best, cand)
out["tune_X"], out["tune_Y"] = Xt, Yt
out["tune_seq"] = seq
out["tune_argmin"] = np.array([dr.K, dr.X_scale, dr.Y_scale])
out["tune_loss"] = np.array(tune_loss)
out["tune_B"] = dr.B
print("tune:", dr.K, dr.X_scale, dr.Y_scale, tune_loss)

np.savez(os.path.join(HERE, "gkdr.npz"), **out)
print("wrote gkdr.npz")
