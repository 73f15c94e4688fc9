"""Host checks of the log-posterior Hessian: the NumPy restatement (tests/hessian_restate.py) against finite differences of the CPU oracle's
gradient, the prior term and the assembly of the block (hessian_assemble) of csrc/hostmath.h against Priors.py and the restatement, and
LaplaceResult on hand-made Hessians.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from numpy.testing import assert_allclose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hessian_restate as hr                                        # noqa: E402
from oracle import cpu_ref as R                                     # noqa: E402
from mogp_emulator_amd.Laplace import LaplaceResult                 # noqa: E402

ORACLE = {"SquaredExponential": R.SQEXP, "Matern52": R.MAT52, "UniformSqExp": R.UNISQEXP, "UniformMat52": R.UNIMAT52}


def _data(n=33, D=3, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.random((n, D))
    t = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + .1 * rng.standard_normal(n)
    return X, t


def _theta(kernel, D):
    corr = [0.3] if kernel in hr.UNIFORM else list(np.linspace(0.3, 1.1, D) * np.where(np.arange(D) % 2, -1., 1.))
    return np.array(corr + [0.2, -4.])


@pytest.mark.parametrize("kernel", sorted(ORACLE))
def test_restatement_matches_finite_differences(kernel):
    """central differences (h = 1e-5) of the oracle's analytic gradient, fitted nugget log eta = -4 (weak priors): 1e-7 of max|H|, 100 x the
    finite difference's own error measured at these shapes (8e-10 / 1.3e-9)"""
    X, t = _data()
    th = _theta(kernel, X.shape[1])
    H = hr.hessian(X, t, th, kernel, nugget_fit=True)
    gp = R.GPRef(X, t, kernel=ORACLE[kernel], nugget="fit")
    h = 1e-5
    F = np.zeros_like(H)
    for j in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        F[:, j] = (gp.logpost_deriv(tp) - gp.logpost_deriv(tm)) / (2 * h)
    err = np.abs(H - F).max() / np.abs(H).max()
    print(kernel, "finite-difference disagreement", err)
    assert err <= 1e-7
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("kernel,nugget", [("SquaredExponential", 1e-4), ("Matern52", 1e-4), ("UniformSqExp", 1e-4)])
def test_restatement_constant_nugget(kernel, nugget):
    """a fixed (or adaptive) nugget is a constant: the Hessian over [corr | cov] against the oracle's gradient with that nugget"""
    X, t = _data()
    th = _theta(kernel, X.shape[1])[:-1]
    H = hr.hessian(X, t, th, kernel, nugget_fit=False, nugget=nugget)
    gp = R.GPRef(X, t, kernel=ORACLE[kernel], nugget=nugget)
    h = 1e-5
    F = np.zeros_like(H)
    for j in range(th.size):
        tp, tm = th.copy(), th.copy()
        tp[j] += h
        tm[j] -= h
        F[:, j] = (gp.logpost_deriv(tp) - gp.logpost_deriv(tm)) / (2 * h)
    # nugget 1e-4 instead of e^-4: the matrix is ~200 x worse conditioned and so is the finite difference (5e-6 measured at 1e-6)
    assert np.abs(H - F).max() / np.abs(H).max() <= 1e-5
    assert np.array_equal(H, H.T)


@pytest.mark.parametrize("uni,per", [("UniformSqExp", "SquaredExponential"), ("UniformMat52", "Matern52")])
def test_uniform_is_block_sum_of_per_dimension(uni, per):
    X, t = _data()
    D = X.shape[1]
    Hu = hr.hessian(X, t, np.array([0.4, 0.2, -4.]), uni, nugget_fit=True)
    Hd = hr.hessian(X, t, np.array([0.4] * D + [0.2, -4.]), per, nugget_fit=True)
    assert_allclose(Hu, hr.uniform_from_per_dimension(Hd, D), rtol=0, atol=1e-11 * np.abs(Hu).max())


def test_long_double_restatement_close():
    X, t = _data()
    th = _theta("Matern52", 3)
    H = hr.hessian(X, t, th, "Matern52", nugget_fit=True)
    HL = hr.hessian(X, t, th, "Matern52", nugget_fit=True, dtype=np.longdouble)
    assert HL.dtype == np.longdouble
    assert float(np.abs(H - HL).max() / np.abs(HL).max()) < 1e-10


def _assemble_inputs(X, t, theta, kernel, nugget_fit, nugget):
    """what the device hands hessian_assemble (the header of csrc/kernels_hess.hip), in float64 NumPy from the definitions: per-dimension
    planes also for a uniform kernel (every e_p = e^theta_0); rows of V, U and z padded with zeros to NPh = n rounded up to 64; the entries
    of T and A the kernels do not write are zero"""
    n, D = X.shape
    uniform = kernel in hr.UNIFORM
    base = hr.UNIFORM[kernel] if uniform else hr.PER_DIM[kernel]
    nc = 1 if uniform else D
    e = np.exp(np.full(D, theta[0]) if uniform else theta[:D])
    sig2 = np.exp(theta[nc])
    eta = float(np.exp(theta[nc + 1])) if nugget_fit else float(nugget)
    s = np.moveaxis((X[:, None, :] - X[None, :, :]) ** 2 * e, -1, 0)         # s_p (D, n, n)
    k, k1, k2 = hr._kernel_derivs(base, s.sum(0), np.float64)
    eye = np.eye(n)
    Qi = hr.chol_inverse(sig2 * k + eta * eye)
    a = Qi @ t
    W = Qi - np.outer(a, a)
    M = [Qi @ (sig2 * k1 * s[p]) for p in range(D)]                          # M_p = Q^-1 Q_p
    o = np.array([0.5 * np.sum(W * sig2 * k1 * s[p]) for p in range(D)] + [0.5 * np.sum(W * sig2 * k), np.trace(Qi), a @ a])
    planes = M + [Qi, eye]
    T = np.zeros((D + 1, D + 2))
    for p in range(D):
        for q in range(p, D + 2):
            T[p, q] = np.sum(planes[p] * planes[q].T)
    T[D, D] = np.sum(Qi * Qi.T)
    A = np.zeros((D, D))
    for p in range(D):
        for q in range(p, D):
            A[p, q] = np.sum(W * sig2 * k2 * s[p] * s[q])        # (the lower triangle twice and the diagonal once: the whole matrix)
    NPh = -(-n // 64) * 64
    V, U, z = np.zeros((D, NPh)), np.zeros((D, NPh)), np.zeros(NPh)
    for p in range(D):
        V[p, :n] = M[p].T @ t
        U[p, :n] = M[p] @ a
    z[:n] = Qi @ a
    return dict(n=n, D=D, NC=nc, uniform=int(uniform), nug_fit=int(nugget_fit), NPh=NPh, eta=eta, o=o, T=T, A=A, V=V, U=U, z=z, alpha=a, t=t)


def _case_text(c, dpr):
    arrays = [c[k] for k in ("o", "T", "A", "V", "U", "z", "alpha", "t")] + [np.asarray(dpr, dtype=float)]
    return "%d %d %d %d %d %d %.17g\n" % (c["n"], c["D"], c["NC"], c["uniform"], c["nug_fit"], c["NPh"], c["eta"]) + \
        "".join(" ".join("%.17g" % x for x in np.ravel(a)) + "\n" for a in arrays)


def _run_assemble(exe, tmp_path, texts):
    """the blocks of the cases of `texts`: (finite flag, P x P array) each"""
    path = tmp_path / "cases.txt"
    path.write_text("".join(texts))
    it = iter(subprocess.check_output([exe, str(path)]).decode().splitlines())
    out = []
    for head in it:
        flag, P = head.split()
        out.append((flag == "ok", np.array([[float(x) for x in next(it).split()] for _ in range(int(P))])))
    assert len(out) == len(texts)
    return out


ASSEMBLE_CASES = [(kernel, D, nug) for D in (3, 1) for kernel in ("SquaredExponential", "Matern52") for nug in ("fit", 1e-4)] + \
                 [("UniformSqExp", 3, "fit"), ("UniformSqExp", 3, 1e-4), ("UniformMat52", 3, "fit"), ("UniformMat52", 3, 1e-4),
                  ("Matern52", 3, "fit-priors")]


def test_hessian_assemble_matches_long_double_restatement(tmp_path):
    """hessian_assemble (csrc/hostmath.h), compiled for the host and fed the device's sums as float64 NumPy computes them from their
    definitions, against the long-double restatement.  The bar per case: 100 x the disagreement of the float64 restatement with the
    long-double one, relative to max|H|; a case whose own disagreement exceeds 1e-8 is refused as ill-conditioned.  Measured (n = 33):
    the float64 restatement disagrees by 9e-15 .. 1e-10 (the largest at the constant nugget 1e-4), the assembled block by 0.6 .. 11.4 x
    that (DESIGN.md section 4 has every figure).  The block is exactly symmetric after the caller's mirror write, and a NaN in any input gives `false`."""
    from test_host_boundary import _build_host_check
    from mogp_emulator_amd.Priors import InvGammaPrior, GammaPrior, LogNormalPrior
    from mogp_emulator_amd.libgpgpu import CorrTransform, CovTransform
    exe = _build_host_check(tmp_path, "hessian_assemble_check")
    cases, texts, wants, own = [], [], [], []
    for kernel, D, nug in ASSEMBLE_CASES:
        X, t = _data()
        X = X[:, :D]                      # (D = 1: the targets keep the part the other inputs explain; data is data)
        fit = nug != 1e-4
        th = _theta(kernel, D)
        th = th if fit else th[:-1]
        dpr = np.zeros(th.size)
        if nug == "fit-priors":
            pri = [InvGammaPrior(2.5, 0.7), GammaPrior(3., 0.4), LogNormalPrior(0.8, 1.3)]
            dpr = np.array([p.d2logpdtheta2(float(np.exp(-0.5 * x)), CorrTransform()) for p, x in zip(pri, th)] +
                           [GammaPrior(2., 1.5).d2logpdtheta2(float(np.exp(th[D])), CovTransform()),
                            InvGammaPrior(1.5, 1e-2).d2logpdtheta2(float(np.exp(th[D + 1])), CovTransform())])
            assert np.all(dpr != 0.)
        kw = dict(nugget_fit=fit, nugget=None if fit else nug, prior_d2=dpr)
        HL = hr.hessian(X, t, th, kernel, dtype=np.longdouble, **kw)
        H64 = hr.hessian(X, t, th, kernel, **kw)
        cases.append(_assemble_inputs(X, t, th, kernel, fit, None if fit else nug))
        texts.append(_case_text(cases[-1], dpr))
        wants.append(HL)
        own.append(float(np.abs(H64 - HL).max() / np.abs(HL).max()))
    got = _run_assemble(exe, tmp_path, texts)
    for (kernel, D, nug), HL, d64, (finite, H) in zip(ASSEMBLE_CASES, wants, own, got):
        err = float(np.abs(H - HL).max() / np.abs(HL).max())
        print("%-18s D=%d nugget=%-10s float64 restatement %.2e  assembled %.2e  (%.1f x)" % (kernel, D, nug, d64, err, err / d64))
        assert d64 <= 1e-8, "ill-conditioned case"
        assert finite
        assert H.shape == HL.shape and err <= 100 * d64, (kernel, D, nug, err, d64)
        assert np.array_equal(H, H.T)
    # a NaN in any input: false, and the caller leaves the block NaN (fitted nugget: every one of them reaches the block)
    base = cases[ASSEMBLE_CASES.index(("Matern52", 3, "fit"))]
    bad = []
    for key, at in (("o", 0), ("o", 3), ("o", 4), ("o", 5), ("T", (0, 1)), ("T", (1, 4)), ("T", (3, 3)), ("A", (1, 2)), ("V", (2, 7)), ("U", (1, 32)),
                    ("z", 5), ("alpha", 0), ("t", 32), ("eta", None), ("dpr", 4)):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        dpr = np.zeros(5)
        if key == "eta":
            c["eta"] = np.nan
        elif key == "dpr":
            dpr[at] = np.nan
        else:
            c[key][at] = np.nan
        bad.append(_case_text(c, dpr))
    for finite, H in _run_assemble(exe, tmp_path, bad):
        assert not finite and np.all(np.isnan(H))


def test_hostmath_prior_second_derivative_matches_python(tmp_path):
    """Priors::d2logpdtheta2 (csrc/hostmath.h), compiled for the host, against Priors.py's d2logpdtheta2 for every family"""
    from mogp_emulator_amd.Priors import InvGammaPrior, GammaPrior, LogNormalPrior, WeakPrior
    from mogp_emulator_amd.libgpgpu import CorrTransform, CovTransform
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "prior_d2_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mogp_emulator_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "prior_d2_check.cpp"), "-o", exe])
    code = {InvGammaPrior: 0, GammaPrior: 1, LogNormalPrior: 2}
    corr = [InvGammaPrior(2.5, 0.7), GammaPrior(3., 0.4), LogNormalPrior(0.8, 1.3), WeakPrior()]
    cov, nug = GammaPrior(2., 1.5), InvGammaPrior(1.5, 1e-2)
    theta = np.array([0.3, -0.8, 1.4, 0.1, 0.6, -4.])

    def spec(p):
        return "%d %.17g %.17g" % ((code[type(p)], p.shape, p.scale) if type(p) in code else (3, 0., 0.))
    for nug_type, nd in ((1, 6), (2, 5)):
        text = "%d %d\n%s\n%s\n" % (len(corr), nug_type, "\n".join(spec(p) for p in corr + [cov, nug]), " ".join("%.17g" % x for x in theta))
        got = np.array(subprocess.check_output([exe], input=text.encode()).decode().split(), dtype=float)
        want = [p.d2logpdtheta2(float(np.exp(-0.5 * th)), CorrTransform()) for p, th in zip(corr, theta)]
        want.append(cov.d2logpdtheta2(float(np.exp(theta[4])), CovTransform()))
        if nug_type == 1:
            want.append(nug.d2logpdtheta2(float(np.exp(theta[5])), CovTransform()))
        assert got.shape == (nd,)
        assert_allclose(got, want, rtol=1e-13, atol=0)
        assert got[3] == 0.


def test_laplace_result_positive_definite():
    H = np.array([[4., 1.], [1., 3.]])
    r = LaplaceResult([0.5, -1.], H)
    assert r.is_minimum
    assert_allclose(r.covariance, np.linalg.inv(H), rtol=1e-14)
    assert_allclose(r.stderr, np.sqrt(np.diag(np.linalg.inv(H))), rtol=1e-14)
    draws = r.sample(200000, rng=1)
    assert draws.shape == (200000, 2)
    assert_allclose(draws.mean(0), [0.5, -1.], atol=5e-3)
    assert_allclose(np.cov(draws.T), np.linalg.inv(H), atol=5e-3)
    assert np.array_equal(r.sample(3, rng=7), r.sample(3, rng=np.random.default_rng(7)))


def test_laplace_result_indefinite():
    r = LaplaceResult([0., 0.], np.array([[1., 2.], [2., 1.]]))
    assert not r.is_minimum
    assert_allclose(r.eigenvalues, [-1., 3.], atol=1e-14)
    assert np.all(np.isnan(r.covariance)) and np.all(np.isnan(r.stderr))
    with pytest.raises(ValueError):
        r.sample(1)
    with pytest.raises(ValueError):
        LaplaceResult([0., 0.], np.eye(3))
