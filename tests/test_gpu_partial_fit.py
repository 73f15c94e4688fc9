"""A partly fitted MultiOutputGP_GPU whose fitted emulators are no leading block: 5 emulators, 1 and 3 not fit, as one part and as
devices=[0, 0] (whose second part holds rows 3 and 4: an unfitted row in front of a fitted one).  The library runs the fitted emulators
of a part on compact rows and scatters the results (csrc/fitted_rows.h); every call that does so is checked here at the smallest shape
where the scatter can go wrong -- rows of unfitted emulators untouched / NaN / 0, fitted rows what the emulator's own call gives, and
the same bits from one part and from two."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd.Priors import GPPriors

pytestmark = pytest.mark.gpu

NE, N, D, M_PTS, S, N_BASE = 5, 33, 3, 9, 3, 64
FIT, UNFIT = [0, 2, 4], [1, 3]
SENT = -123.25
DOUBLES = ("mean", "var", "deriv", "fc_mean", "fc_cov", "sobol_S", "sobol_ST", "sobol_mean", "sobol_var", "sobol_emvar") + tuple(
    "mix_%s_%s" % (kind, name) for kind in ("w", "q") for name in ("mean", "within", "between", "weights", "logpost"))


def inputs():
    rng = np.random.default_rng(7)
    X = rng.random((N, D))
    T = np.stack([np.sin(3 * X[:, 0] + .3 * k) + X[:, 1] ** 2 + .1 * rng.standard_normal(N) for k in range(NE)])
    th = np.array([[1., .5, -.5, .1]]) + .1 * np.arange(NE)[:, None]                       # three correlation lengths, sigma^2
    thetas = th[:, None, :] + .2 * rng.standard_normal((NE, S, D + 1))
    w = .2 + 3. * rng.random((NE, S))
    w[:, 1] = 0.                                                                          # one exact zero per emulator
    return dict(X=X, T=T, Xs=rng.random((M_PTS, D)), th=th, thetas=thetas, w=w, q=rng.standard_normal((NE, S)),
                A=rng.random((N_BASE, D)), B=rng.random((N_BASE, D)))


def model(devices=None, fit=FIT):
    c = inputs()
    mo = M.MultiOutputGP_GPU(c["X"], c["T"], kernel="Matern52", nugget=1e-4, priors=GPPriors(n_corr=D, nugget_type="fixed"), devices=devices)
    for k in fit:
        mo.fit_emulator(k, c["th"][k])
    return mo, c


def calls(lib, c, shape=()):
    """every call that goes through the compact rows, on the multi-output shim (shape = (NE,)) or on one emulator's (shape = ())"""
    Xs, out = c["Xs"], {}
    out["mean"], out["var"] = np.full(shape + (M_PTS,), SENT), np.full(shape + (M_PTS,), SENT)
    lib.predict_variance_batch(Xs, out["mean"], out["var"])
    out["deriv"] = np.full(shape + (M_PTS, D), SENT)
    lib.predict_deriv(Xs, out["deriv"])
    out["fc_mean"], out["fc_cov"] = np.full(shape + (M_PTS,), SENT), np.full(shape + (M_PTS, M_PTS), SENT)
    lib.predict_full_cov(Xs, out["fc_mean"], out["fc_cov"])
    for k, a in zip(("S", "ST", "mean", "var", "emvar"), lib.sobol(c["A"], c["B"], unc=True)):
        out["sobol_" + k] = np.asarray(a)
    e = c.get("emulator")
    for kind, kw in (("w", "weights"), ("q", "log_q")):
        got = lib.predict_mixture(c["thetas"] if e is None else c["thetas"][e], Xs, **{kw: c[kind] if e is None else c[kind][e]})
        for k, a in zip(("mean", "within", "between", "weights", "logpost", "ok", "ok_all"), got):
            out["mix_%s_%s" % (kind, k)] = a
    return out


def outputs(devices=None):
    mo, c = model(devices)
    assert mo._mogp_gpu.parts() == ([(0, 0, 3), (0, 3, 5)] if devices else [(0, 0, NE)])
    assert mo.get_indices_fit() == FIT and mo.get_indices_not_fit() == UNFIT
    return mo, c, calls(mo._mogp_gpu, c, (NE,))


def test_non_contiguous_fitted_rows():
    runs = {None: outputs(), (0, 0): outputs([0, 0])}                                    # computed once, shared by everything below
    one, two = runs[None][2], runs[(0, 0)][2]
    for tag, out in (("one part", one), ("two parts", two)):
        for k in ("mean", "var", "deriv", "fc_mean", "fc_cov"):
            assert np.all(out[k][UNFIT] == SENT), (tag, k)
            assert np.all(np.isfinite(out[k][FIT])) and not np.any(out[k][FIT] == SENT), (tag, k)
        for k in DOUBLES[5:]:
            assert np.all(np.isnan(out[k][UNFIT])), (tag, k)
            assert np.all(np.isfinite(out[k][FIT])), (tag, k)
        for kind in ("w", "q"):
            assert not out["mix_%s_ok" % kind][UNFIT].any() and not out["mix_%s_ok_all" % kind][UNFIT].any(), (tag, kind)
            assert out["mix_%s_ok" % kind][FIT].all() and out["mix_%s_ok_all" % kind][FIT].all(), (tag, kind)
    assert sorted(one) == sorted(two)
    for k in sorted(one):
        assert np.array_equal(one[k], two[k], equal_nan=one[k].dtype.kind == "f"), k
    # every fitted row against the emulator's own call: equal, variances to 1e-15 (the bars of test_gpu_multidevice.py, test_gpu_sobol.py
    # and test_gpu_marginal.py::test_multi_output)
    for devices, (mo, c, out) in runs.items():
        for i in FIT:
            own = calls(mo._mogp_gpu.emulator(i), dict(c, emulator=i))
            for k in sorted(own):
                a, b = out[k][i], own[k]
                if k in ("var", "fc_cov", "sobol_emvar"):
                    print(devices, i, k, "max |d| %.3g, relative %.3g" % (np.max(np.abs(a - b)), np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
                    assert_allclose(a, b, rtol=1e-15, atol=0, err_msg="%s emulator %d %s" % (devices, i, k))
                    assert_allclose(a, b, rtol=0, atol=1e-15, err_msg="%s emulator %d %s" % (devices, i, k))
                else:
                    assert np.array_equal(a, b), (devices, i, k)
