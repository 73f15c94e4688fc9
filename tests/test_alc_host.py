"""Host-side checks of the active-learning module: the argument refusals that need no device, the arithmetic of ALCResult, alc_plan
(csrc/predict_plan.h) against a hand-worked table through a sanitised host program, ALCDesign's bookkeeping, and the NumPy restatement
(alc_restate.py) in float64 against itself in long double on the shapes of the GPU tests -- which proves that the bars the device is held
to are not vacuous: the float64 error lies below them and above 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mogp_emulator_amd as M
from mogp_emulator_amd import ActiveLearning, LibGPGPU

import alc_restate as ar

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


def test_alc_plan_matches_the_hand_worked_table(tmp_path):
    out = _build_and_run(tmp_path, "alc_plan_check")
    assert out.strip() == "ok 11 rows"


def test_exports():
    assert M.alc_criterion is ActiveLearning.alc_criterion and M.predict_cov is ActiveLearning.predict_cov
    assert M.ALCResult is ActiveLearning.ALCResult
    if LibGPGPU.HAVE_LIBGPGPU:
        from mogp_emulator_amd.SequentialDesign import ALCDesign, SequentialDesign
        assert M.ALCDesign is ALCDesign and issubclass(ALCDesign, SequentialDesign)


def test_not_a_gpu_emulator_is_refused():
    X = np.zeros((4, 2))
    for bad in (None, object(), np.zeros(3), "gp"):
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.alc_criterion(bad, X, X)
        with pytest.raises(TypeError, match="needs a GaussianProcessGPU or a MultiOutputGP_GPU"):
            M.predict_cov(bad, X)


class _FakeNative(object):
    def __init__(self, fit):
        self.fit = fit
        self.calls = 0

    def theta_fit_status(self):
        return self.fit

    def alc(self, *a, **k):
        self.calls += 1
        raise AssertionError("the device must not be reached")

    predict_cov = alc


def _fake_gp(monkeypatch, D=3, nugget_type="fixed", analytic=False, fit=True):
    """An object that passes for a GaussianProcessGPU in the shim's checks without touching a device"""
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
    gp._densegp_gpu = _FakeNative(fit)
    return gp


@pytest.mark.skipif(not LibGPGPU.HAVE_LIBGPGPU, reason="the library is not built")
def test_refusals_come_before_any_device_call(monkeypatch):
    gp = _fake_gp(monkeypatch)
    X, R = np.random.default_rng(0).random((5, 3)), np.random.default_rng(1).random((7, 3))
    bad_points = [np.zeros((5, 2)), np.zeros((0, 3)), np.zeros((2, 3, 1))]
    for b in bad_points:
        with pytest.raises(ValueError, match="must have shape"):
            M.alc_criterion(gp, b, R)
        with pytest.raises(ValueError, match="must have shape"):
            M.alc_criterion(gp, X, b)
        with pytest.raises(ValueError, match="must have shape"):
            M.predict_cov(gp, b)
        with pytest.raises(ValueError, match="must have shape"):
            M.predict_cov(gp, X, b)
    for v in (np.nan, np.inf):
        Xb = X.copy()
        Xb[2, 1] = v
        with pytest.raises(ValueError, match="must be finite"):
            M.alc_criterion(gp, Xb, R)
        with pytest.raises(ValueError, match="must be finite"):
            M.alc_criterion(gp, X, R, weights=np.r_[v, np.ones(6)])
        with pytest.raises(ValueError, match="must be finite"):
            M.predict_cov(gp, X, Xb)
        with pytest.raises(ValueError, match="noise must be a finite number that is not negative"):
            M.alc_criterion(gp, X, R, noise=v)
    with pytest.raises(ValueError, match="weights must have shape"):
        M.alc_criterion(gp, X, R, weights=np.ones(6))
    with pytest.raises(ValueError, match="weights must not be negative"):
        M.alc_criterion(gp, X, R, weights=np.r_[-1e-300, np.ones(6)])
    with pytest.raises(ValueError, match="weights must not sum to 0"):
        M.alc_criterion(gp, X, R, weights=np.zeros(7))
    with pytest.raises(ValueError, match="noise must be a finite number that is not negative"):
        M.alc_criterion(gp, X, R, noise=-1e-12)
    with pytest.raises(ValueError, match="max_slots and max_points must not be negative"):
        M.alc_criterion(gp, X, R, max_slots=-1)
    with pytest.raises(ValueError, match="max_slots and max_points must not be negative"):
        M.alc_criterion(gp, X, R, max_points=-128)
    with pytest.raises(ValueError, match="max_slots and max_points must not be negative"):
        M.predict_cov(gp, X, max_slots=-1)
    for kw, msg in ((dict(nugget_type="pivot"), 'not available with nugget="pivot"'), (dict(analytic=True), "not available with analytic_mean=True"),
                    (dict(fit=False), "hyperparameters have not been fit")):
        g = _fake_gp(monkeypatch, **kw)
        with pytest.raises(RuntimeError, match=msg):
            M.alc_criterion(g, X, R)
        with pytest.raises(RuntimeError, match=msg):
            M.predict_cov(g, X, R)
        assert g._densegp_gpu.calls == 0
    assert gp._densegp_gpu.calls == 0


def test_alc_result_arithmetic():
    red = np.array([[1., 4., 2., 4.], [np.nan] * 4, [.5, .25, 3., 0.]])
    rv = np.array([[2., 4.], [np.nan, np.nan], [1., 3.]])
    w = np.array([.25, .75])
    r = M.ALCResult(reduction=red, cand_variance=np.zeros((3, 4)), ref_variance=rv, degenerate=np.zeros((3, 4), dtype=bool), noise=np.zeros(3), weights=w)
    iv = r.integrated_variance
    assert iv.shape == (3,) and iv[0] == 3.5 and np.isnan(iv[1]) and iv[2] == 2.5
    assert r.best.tolist() == [1, 0, 2]                      # the first of equal maxima; 0 for the emulator that is not fit
    np.testing.assert_array_equal(r.total(scale=False), [1.5, 4.25, 5., 4.])
    np.testing.assert_array_equal(r.total(), red[0] / 3.5 + red[2] / 2.5)
    assert r.total().shape == (4,)


@pytest.mark.skipif(not LibGPGPU.HAVE_LIBGPGPU, reason="the library is not built")
def test_alc_design_bookkeeping(tmp_path):
    from mogp_emulator_amd import ALCDesign, LatinHypercubeDesign
    base = LatinHypercubeDesign(2)
    with pytest.raises(ValueError, match="reference points must be positive"):
        ALCDesign(base, n_ref=0)
    with pytest.raises(ValueError, match="nugget parameter cannot be negative"):
        ALCDesign(base, nugget=-1.)
    with pytest.raises(ValueError, match="noise variance cannot be negative"):
        ALCDesign(base, noise=-1.)
    with pytest.raises(TypeError):
        ALCDesign("not a design")
    ad = ALCDesign(base, n_init=4, n_cand=9, n_ref=33, nugget=1e-3, noise=.5)
    assert (ad.get_n_ref(), ad.get_noise(), ad.get_nugget(), ad.get_n_cand(), ad.get_n_init()) == (33, .5, 1e-3, 9, 4)
    np.random.seed(3)
    ad.generate_initial_design()
    ad.set_initial_targets(np.arange(4.))
    ad._generate_candidates()
    ad.save_design(str(tmp_path / "d.npz"))
    for noise in (None, 2.):
        other = ALCDesign(base, n_init=4, n_cand=9, n_ref=5, nugget=1e-3, noise=noise)
        other.load_design(str(tmp_path / "d.npz"))
        assert other.get_n_ref() == 33 and other.get_noise() == .5 and other.get_current_iteration() == 4
        assert np.array_equal(other.get_inputs(), ad.get_inputs()) and np.array_equal(other.get_candidates(), ad.get_candidates())
    nn = ALCDesign(base, n_init=4, n_cand=9)
    nn.generate_initial_design()
    nn.save_design(str(tmp_path / "n.npz"))
    back = ALCDesign(base, n_init=4, n_cand=9, noise=1.)
    back.load_design(str(tmp_path / "n.npz"))
    assert back.get_noise() is None and back.get_n_ref() == 200
    if not LibGPGPU.gpu_usable():
        with pytest.raises(RuntimeError, match="Cannot run an ALCDesign step"):
            ad._eval_metric()


# ---- the restatement against itself in long double: the shapes and hyperparameters of tests/test_gpu_alc.py ---------------------------

N, D = 130, 3


def _theta(e, fit):
    corr = np.log(1. / D) + np.linspace(1.0, 3.2, D) + 0.05 * e
    return np.concatenate([corr, [0.2 + 0.03 * e], [-4. + 0.1 * e] if fit else []])


@pytest.mark.skipif(np.finfo(np.longdouble).eps >= 2. ** -60, reason="long double is no wider than double here")
@pytest.mark.parametrize("kind", ("SquaredExponential", "Matern52"))
@pytest.mark.parametrize("fit", (False, True), ids=("fixed", "fit"))
def test_float64_restatement_lies_inside_its_bars_and_is_not_exact(kind, fit):
    rng = np.random.default_rng(77)
    X = rng.random((N, D))
    cand, ref = np.random.default_rng(629).random((129, D)), np.random.default_rng(800).random((300, D))
    e = 1
    th = _theta(e, fit)
    eta = np.exp(th[-1]) if fit else 1e-2
    p64, p80 = ar.Posterior(X, th, kind, eta), ar.Posterior(X, th, kind, eta, dtype=np.longdouble)
    C64, C80 = p64.cov(cand, ref), p80.cov(cand, ref)
    bar = p64.cov_bar(cand, ref)
    err = np.abs(np.asarray(C80 - C64.astype(np.longdouble), dtype=np.float64))
    print("%s %s: float64 cross covariance off by at most %.3g of the bar (cond %.3g)" % (kind, "fit" if fit else "fixed", np.max(err / bar),
                                                                                         np.linalg.cond(p64.Q)))
    assert np.all(err <= bar) and np.max(err) > 0.
    w = np.full(300, 1. / 300)
    a64, _, _, deg, Cc, d = ar.alc(p64, cand, ref, w, eta)
    a80 = ar.alc(p80, cand, ref, w, eta)[0]
    abar = ar.alc_bar(p64, cand, ref, w, Cc, d)
    aerr = np.abs(np.asarray(a80 - a64.astype(np.longdouble), dtype=np.float64))
    print("    ALC off by at most %.3g of the propagated bar" % np.max(aerr / abar))
    assert not deg.any() and np.all(aerr <= abar) and np.max(aerr) > 0.
    # the definition itself: ALC is the drop of the integrated variance when the candidate joins the design with noise tau
    i = int(np.argmax(a80))
    Xp = np.vstack([X, cand[i:i + 1]])
    pp = ar.Posterior(Xp, th, kind, eta, dtype=np.longdouble)
    drop = (p80.var(ref) - pp.var(ref)) @ w.astype(np.longdouble)
    assert abs(float(drop - a80[i])) <= 1e-12 * float(a80[i]) + 1e-15
