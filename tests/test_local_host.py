"""Host-side checks of local approximate GP prediction (mogp_emulator_amd.LocalGP): the argument refusals that need no device, the
bookkeeping of LocalPrediction, local_plan (csrc/predict_plan.h) against a hand-worked table and the named refusals and the LDS layout of
the handle (tests/c/local_args_check.cpp), each through a sanitised stand-alone program, and the NumPy restatement (local_restate.py) in
float64 against itself in long double on every shape of the GPU tests -- which proves that the bars the device is held to are not vacuous:
the float64 error lies below them and above 0."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU

LG = importlib.import_module("mogp_emulator_amd.LocalGP")      # the module: the package exports the class under the same name

import dimension_cases as dc
import local_cases as lc
import local_restate as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"), os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_local_plan_matches_the_hand_worked_table(tmp_path):
    out = _build_and_run(tmp_path, "local_plan_check")
    assert out.strip() == "ok 10 rows"


def test_named_refusals_and_lds_layout_of_the_handle(tmp_path):
    out = _build_and_run(tmp_path, "local_args_check")
    assert out.strip() == "ok 805 checks"


def test_exports():
    assert M.LocalGP is LG.LocalGP and M.predict_local is LG.predict_local and M.LocalPrediction is LG.LocalPrediction
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd import _capi
        for name in ("mogp_local_create", "mogp_local_predict", "mogp_local_destroy"):
            assert name in _capi.SIGNATURES
        assert hasattr(LibGPGPU, "LocalGP_GPU")


def test_not_a_gpu_emulator_is_refused():
    X = np.zeros((4, 2))
    for bad in (None, object(), np.zeros(3), "gp"):
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.LocalGP(bad, X, np.zeros(4))
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.predict_local(bad, X, np.zeros(4), X)


class _FakeNative(object):
    """stands for the fitted native emulator; anything that would go to the device is an error"""

    def __init__(self, fit, kernel, D):
        self.fit, self.kernel, self.D = fit, kernel, D
        self.calls = 0

    def theta_fit_status(self):
        return self.fit

    def get_kernel_type(self):
        return getattr(LibGPGPU.kernel_type, self.kernel)

    def get_theta(self):
        nc = 1 if self.kernel.startswith("Uniform") else self.D
        th = LibGPGPU.GPParameters(0, nc, LibGPGPU.nugget_type.fixed, 1e-2)
        th.set_data(np.r_[np.linspace(-0.3, 0.4, nc), 0.1])
        return th

    def get_nugget_size(self):
        return 1e-2

    def get_meanfunc(self):
        return None

    def predict(self, *a, **k):
        self.calls += 1
        raise AssertionError("the device must not be reached")

    predict_variance_batch = predict_batch = fit_emulator = predict


class _FakeLocalNative(object):
    calls = 0

    def predict(self, *a, **k):
        _FakeLocalNative.calls += 1
        raise AssertionError("the device must not be reached")

    def close(self):
        pass


def _fake_gp(D=3, nugget_type="fixed", analytic=False, fit=True, kernel="SquaredExponential"):
    """An object that passes for a GaussianProcessGPU in the checks without touching a device"""
    from mogp_emulator_amd.GaussianProcessGPU import GaussianProcessGPU

    class Fake(GaussianProcessGPU):
        def __init__(self):                       # no native handle
            pass
        D = property(lambda self: D)
        nugget_type = property(lambda self: nugget_type)
        nugget = property(lambda self: 1e-2)

        def __del__(self):
            pass
    gp = Fake()
    gp._analytic_mean = analytic
    gp._densegp_gpu = _FakeNative(fit, kernel, D)
    return gp


@pytest.mark.skipif(not LibGPGPU.HAVE_LIBGPGPU, reason="the library is not built")
def test_refusals_come_before_any_device_call(monkeypatch):
    created = []

    def no_device(inputs, residuals, device):
        created.append((inputs.shape, residuals.shape, device))
        return _FakeLocalNative()
    monkeypatch.setattr(LG, "_create_native", no_device)
    rng = np.random.default_rng(0)
    X, t, Q = rng.random((9, 3)), rng.random(9), rng.random((4, 3))
    gp = _fake_gp()
    # the design
    for b in (np.zeros((9, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="inputs must have shape"):
            M.LocalGP(gp, b, t)
    for bad_t in (np.zeros(8), np.zeros((2, 9)), np.zeros((9, 1))):
        with pytest.raises(ValueError, match="targets must have shape"):
            M.LocalGP(gp, X, bad_t)
    for v in (np.nan, np.inf):
        Xb, tb = X.copy(), t.copy()
        Xb[2, 1], tb[3] = v, v
        with pytest.raises(ValueError, match="inputs must be finite"):
            M.LocalGP(gp, Xb, t)
        with pytest.raises(ValueError, match="targets must be finite"):
            M.LocalGP(gp, X, tb)
    for k in (0, -1, 10, 127, 2.5):
        with pytest.raises(ValueError, match="n_neighbours must be between 1 and"):
            M.LocalGP(gp, X, t, n_neighbours=k)
    big = rng.random((200, 3))
    with pytest.raises(ValueError, match=r"n_neighbours must be between 1 and min\(N, 126\) = 126"):
        M.LocalGP(gp, big, rng.random(200), n_neighbours=127)
    with pytest.raises(ValueError, match="device must be"):
        M.LocalGP(gp, X, t, n_neighbours=3, device=-1)
    # the emulator
    for kw, msg in ((dict(nugget_type="pivot"), 'not available with nugget="pivot"'), (dict(analytic=True), "not available with analytic_mean=True"),
                    (dict(fit=False), "hyperparameters have not been fit"), (dict(kernel="ProductMat52"), "not available with the ProductMat52 kernel")):
        g = _fake_gp(**kw)
        with pytest.raises(RuntimeError, match=msg):
            M.LocalGP(g, X, t, n_neighbours=3)
        with pytest.raises(RuntimeError, match=msg):
            M.predict_local(g, X, t, Q, n_neighbours=3)
        assert g._densegp_gpu.calls == 0
    assert created == []
    # predict
    for kernel in ("SquaredExponential", "UniformMat52"):
        lg = M.LocalGP(_fake_gp(kernel=kernel), X, t, n_neighbours=3, device=None)
        assert (lg.n, lg.D, lg.n_emulators, lg.n_neighbours) == (9, 3, 1, 3)
        s = lg._hyper[0][1]
        assert s.shape == (3,) and (np.all(s == s[0]) if kernel == "UniformMat52" else len(set(s)) == 3)
    assert created == [((9, 3), (1, 9), None)] * 2
    for b in (np.zeros((4, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError, match="testing must have shape"):
            lg.predict(b)
    Qb = Q.copy()
    Qb[0, 0] = np.nan
    with pytest.raises(ValueError, match="testing must be finite"):
        lg.predict(Qb)
    for j in (-1e-300, np.nan, np.inf):
        with pytest.raises(ValueError, match="jitter must be a finite number that is not negative"):
            lg.predict(Q, jitter=j)
    with pytest.raises(ValueError, match="max_points must not be negative"):
        lg.predict(Q, max_points=-1)
    assert _FakeLocalNative.calls == 0 and gp._densegp_gpu.calls == 0
    lg.close()
    with pytest.raises(RuntimeError, match="has been closed"):
        lg.predict(Q)
    lg.close()                                    # twice is fine


def test_local_prediction_bookkeeping():
    ok = np.array([[True, False, True], [False, False, True]])
    mean = np.where(ok, 1., np.nan)
    p = M.LocalPrediction(mean, None, ok, np.ones((2, 3)), None)
    assert p.n_failed == 3 and p.unc is None and p.neighbours is None and p.mean is mean
    q = M.LocalPrediction(np.zeros(4), np.zeros(4), np.ones(4, dtype=bool), np.zeros(4), np.zeros((4, 2), dtype=np.int64))
    assert q.n_failed == 0 and q.neighbours.dtype == np.int64


def test_restatement_reproduces_the_lattice_ties():
    """the lists of the tie test of test_gpu_local.py, from the restatement: small integers and halves, exact"""
    lat = np.array([[i, j] for i in range(12) for j in range(12)], dtype=float)
    one = np.ones(2)
    for q, k, want in (((5.5, 5.5), 2, [65, 66]), ((5.5, 5.5), 3, [65, 66, 77]), ((5.5, 5.5), 4, [65, 66, 77, 78]), ((5, 5), 3, [65, 53, 64]),
                       ((5, 5), 5, [65, 53, 64, 66, 77])):
        nbr, radius, _ = lr.neighbours(lat, np.array([q], dtype=float), one, k)
        assert nbr[0].tolist() == want


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
@pytest.mark.parametrize("N,D,k,kernel", lc.ALL, ids=lambda v: str(v))
def test_float64_restatement_lies_inside_the_bars_and_is_not_exact(N, D, k, kernel):
    c, (s,) = lc.setup(N, D, kernel)
    ref = lc.reference(N, D, k, kernel)
    m80, v80, ok80, _ = lr.predict(c.X, c.T[0], c.Xs, s, kernel, lc.SIGMA2, dc.NUGGET, ref["nbr"], dtype=np.longdouble)
    assert ok80.all()
    em = np.abs(np.asarray(m80 - ref["mean"].astype(np.longdouble), dtype=np.float64))
    ev = np.abs(np.asarray(v80 - ref["var"].astype(np.longdouble), dtype=np.float64))
    # a principal sub-matrix of K + nugget I: never worse conditioned than the whole, and far from where the bars widen
    srt = np.sort(ref["r2"], axis=1)
    gap = np.min((srt[:, k] - srt[:, k - 1]) / srt[:, k - 1]) if k < N else np.inf
    print("N %d D %d k %d %s: float64 off by at most %.3g (mean) %.3g (variance), cond at most %.3g, smallest relative gap %.3g"
          % (N, D, k, kernel, em.max(), ev.max(), ref["cond"].max(), gap))
    assert ref["cond"].max() <= 1.2e6
    assert em.max() > 0. and lc.excess_rows("mean", ref["mean"], np.asarray(m80, dtype=np.float64), ref["cond"]) <= 1.
    assert ev.max() > 0. and lc.excess_rows("var", ref["var"], np.asarray(v80, dtype=np.float64), ref["cond"]) <= 1.
    # the neighbour sets do not hinge on the last bit: the k-th and the (k+1)-th distance are many roundings apart
    assert gap > 1e-9
