"""The input dimension D swept across every device path that branches on it, on the MI355X, against the CPU oracle (oracle/cpu_ref.py;
the Hessian and the cross-covariance consumers against their NumPy restatements).  The row axes are pinned elsewhere; here n = 130 (three
training tiles) and n = 7 (one partial tile), m = 37 and 65 test points, and D runs over

  * 16 | 17 and 32 | 33: the prefetch depth of cross_cov_mean_kernel (4, 8, or the synchronous form), whose registers hold exactly
    64 D values at 16 and 32;
  * 5, 13, 29 (D + 3 a multiple of 8), 6 (one past) and 80 (11 flushes): the flush of grad_kernel's sums, eight at a time;
  * 8 and 16: the trailing chunk of grad_lowrank_kernel that holds only the covariance-scale term (nugget="pivot" with a repeat);
  * 2, 5, 6, 33, 80: the plane groups of the Hessian's GEMM (4, 2 or 1 planes, the last group padded);
  * 80: the limit -- predict_deriv_kernel's (192 D + 4160) doubles of LDS sit just under 160 KB there.

Cases: dimension_cases.py (every coordinate has its own scale and length; test_dimension_cases_host.py shows on the CPU that a dropped or a
swapped coordinate moves every quantity compared here by more than 100 x its bar).  Bars: those of tests/tools/fuzz_parity.py, with its
amplification max(1, cond * 1e-7), which is 1 for every case but the pivoted ones (no nugget there); the Hessian, cross-validation,
sampling and mixture cases use the bars of their own test files.  Every test loops over D and reports all mismatches before it fails.
The largest differences measured per quantity and band of D: DESIGN.md section 4."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_allclose

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.Priors import GPPriors
from oracle import cpu_ref as R

import dimension_cases as dc

pytestmark = pytest.mark.gpu
E = 3


@pytest.fixture(autouse=True)
def _need_gpu():
    if not M.gpu_usable():
        pytest.skip("no gfx950 device")


def _band(D):
    return "D<=16" if D <= 16 else ("D17..32" if D <= 32 else "D>32")


class _Tally(object):
    """compares at the fuzz's bars, keeps the largest error per (quantity, band of D), and fails at the end with every mismatch"""

    def __init__(self, what):
        self.what, self.worst, self.bad = what, {}, []

    def check(self, tag, got, want, D, ctx, amp=1., gscale=1.):
        got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
        assert got.shape == want.shape, (ctx, tag, got.shape, want.shape)
        err = float(np.abs(got - want).max())
        units = dc.excess(tag, got, want, amp, gscale)
        key = (tag, _band(D))
        if not self.worst.get(key, (0., 0.))[1] >= units:          # (a NaN replaces whatever is there)
            self.worst[key] = (err, units)
        if not (np.all(np.isfinite(got)) and units <= 1.):
            self.bad.append("MISMATCH %s %s: max abs err %.3e = %.3g x the bar" % (ctx, tag, err, units))
            print(self.bad[-1], flush=True)

    def finish(self):
        for (tag, band), (err, units) in sorted(self.worst.items()):
            rtol, atol = dc.BARS[tag]
            print("sweep %s | %s | %s | max abs err %.3e | %.3g of the bar (rtol %g, atol %g)" % (self.what, tag, band, err, units, rtol, atol))
        assert not self.bad, "%d mismatches:\n%s" % (len(self.bad), "\n".join(self.bad))


def _terms_of(mean, D):
    return {"zero": None, "const": (), "first": ((0, 1),), "last": ((D - 1, 1),)}[mean]


@functools.lru_cache(maxsize=None)
def _oracle_values(n, D, kernel, mean, repeat):
    """per emulator, the oracle's values at m = 65 points (the first 37 are the m = 37 run); computed once, never modified.  With a nugget
    they are computed as a fitted one of log(1e-4) and serve the fixed nugget of 1e-4 too (_reference)."""
    c = dc.case(n, D, kernel, m=max(dc.M_TEST), E=E, fit=not repeat, repeat=repeat)
    if repeat:
        c = c._replace(nugget="pivot")
    terms = _terms_of(mean, D)
    refs = []
    for k in range(E):
        out, ref = dc.oracle(c, k, terms=None if terms is None else list(terms), deriv=terms is None)
        out["K"] = ref.get_K_matrix()
        out["cond"], out["amp"] = dc.amplification(out["K"] + (ref.nugget or 0.) * np.eye(n), int(repeat))
        out["fullcov"] = ref.predict(c.Xs[:9], full_cov=True)[1]
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        refs.append(out)
    return refs


def _reference(n, D, kernel, fit, mean="zero", repeat=False):
    """(case, oracle values per emulator).  A fixed nugget of 1e-4 and a fitted one of log(1e-4) are the same model (the priors are weak;
    exp(log(1e-4)) is 1e-4 to an ulp, 1e-20 in absolute terms): the fixed-nugget gradient is the fitted one without its last entry, and
    everything else is shared -- the oracle of the product kernel at D = 80 takes more than a second per emulator."""
    c = dc.case(n, D, kernel, m=max(dc.M_TEST), E=E, fit=fit, repeat=repeat)
    if repeat:
        c = c._replace(nugget="pivot")
    refs = _oracle_values(n, D, kernel, mean, repeat)
    if not fit and not repeat:
        refs = [dict(r, grad=r["grad"][:-1]) for r in refs]
    return c, refs


def _model(c, D, mean="zero"):
    kw = {}
    terms = _terms_of(mean, D)
    if terms is not None:
        kw = dict(mean=LibGPGPU.PolyMeanFunc(list(terms)) if terms else LibGPGPU.ConstMeanFunc(), analytic_mean=True)
    kind = c.nugget if isinstance(c.nugget, str) else "fixed"
    return M.MultiOutputGP_GPU(c.X, c.T, kernel=c.kernel, nugget=c.nugget, priors=GPPriors(n_corr=c.nc, nugget_type=kind), **kw)


def _check_fit(tally, mo, c, refs, D, ctx):
    f, g, ok = mo._mogp_gpu.eval(c.thetas, grad=True)
    assert ok.all(), ctx
    for k in range(E):
        r = refs[k]
        tally.check("logpost", f[k], r["logpost"], D, "%s emulator %d" % (ctx, k), r["amp"])
        tally.check("grad", g[k], r["grad"], D, "%s emulator %d" % (ctx, k), r["amp"], max(1., float(np.abs(g[k]).max())))


def _check_predict(tally, mo, c, refs, D, ctx, deriv=True):
    for m in dc.M_TEST:
        mean, var, dv = mo.predict(c.Xs[:m], deriv=deriv)
        for k in range(E):
            r, cm = refs[k], "%s m=%d emulator %d" % (ctx, m, k)
            tally.check("mean", mean[k], r["mean"][:m], D, cm, r["amp"])
            tally.check("var", var[k], r["var"][:m], D, cm, r["amp"])
            if deriv:
                tally.check("deriv", dv[k], r["deriv"][:m], D, cm, r["amp"])


def _fit_path(kernel, fit, shapes):
    tally = _Tally("fit %s %s" % (kernel, "fit" if fit else "fixed"))
    for n, Ds in shapes:
        for D in Ds:
            c, refs = _reference(n, D, kernel, fit)
            _check_fit(tally, _model(c, D), c, refs, D, "n=%d D=%d %s" % (n, D, kernel))
    tally.finish()


def _predict_path(kernel, fit, shapes):
    tally = _Tally("predict %s %s" % (kernel, "fit" if fit else "fixed"))
    for n, Ds in shapes:
        for D in Ds:
            c, refs = _reference(n, D, kernel, fit)
            mo = _model(c, D)
            mo.fit(c.thetas)
            _check_predict(tally, mo, c, refs, D, "n=%d D=%d %s" % (n, D, kernel))
            if D in dc.D_EDGES:
                cov = mo.predict(c.Xs[:9], full_cov=True, deriv=False)[1]          # cov_full_kernel over the batch
                for k in range(E):
                    ck = "n=%d D=%d %s emulator %d" % (n, D, kernel, k)
                    tally.check("fullcov", cov[k], refs[k]["fullcov"], D, ck, refs[k]["amp"])
                    # ... and for one emulator: K without the nugget, at the full covariance's bar
                    tally.check("fullcov", mo.emulators[k].get_K_matrix(), refs[k]["K"], D, ck + " K", refs[k]["amp"])
    tally.finish()


# The sweep in four parts, so that no test waits for more than a few seconds of the oracle (its product kernel costs D^2 n^2 per emulator)
PARTS = {"D1-33": [(dc.N_TILES, [D for D in dc.D_SWEEP if D <= 33])], "D48-64": [(dc.N_TILES, [48, 64])], "D79": [(dc.N_TILES, [79])],
         "D80-and-partial-tile": [(dc.N_TILES, [80]), (dc.N_PARTIAL, dc.D_EDGES)]}
assert sorted(D for p in PARTS.values() for n, Ds in p if n == dc.N_TILES for D in Ds) == dc.D_SWEEP
EDGES = [(dc.N_TILES, dc.D_EDGES), (dc.N_PARTIAL, dc.D_EDGES)]
NUGGETS = pytest.mark.parametrize("fit", [False, True], ids=["fixed", "fit"])
SWEEP = pytest.mark.parametrize("part", list(PARTS))


@NUGGETS
@SWEEP
@pytest.mark.parametrize("kernel", dc.PER_DIM)
def test_fit_path(kernel, part, fit):
    """objective and gradient of three emulators with their own theta in one model: cov_build_kernel, grad_kernel, the P / X strides"""
    _fit_path(kernel, fit, PARTS[part])


@NUGGETS
@pytest.mark.parametrize("kernel", dc.UNIFORM)
def test_fit_path_uniform_kernels(kernel, fit):
    _fit_path(kernel, fit, EDGES)


@NUGGETS
@SWEEP
@pytest.mark.parametrize("kernel", dc.PER_DIM)
def test_predict_path(kernel, part, fit):
    """mean, variance and input derivative after fit(theta), in all three prefetch forms of the cross covariance; the full covariance and
    K itself at the edges"""
    _predict_path(kernel, fit, PARTS[part])


@NUGGETS
@pytest.mark.parametrize("kernel", dc.UNIFORM)
def test_predict_path_uniform_kernels(kernel, fit):
    _predict_path(kernel, fit, EDGES)


@pytest.mark.parametrize("mean", ["const", "first", "last"])
@pytest.mark.parametrize("kernel", dc.PER_DIM)
def test_analytic_mean(kernel, mean):
    """a constant, and an intercept with a slope along the first / the last coordinate, integrated out: the RB = RMAX family of the cross
    covariance at prefetch depths 4 (D = 5, 16), 8 (17, 32) and 0 (33, 80); fitted nugget"""
    tally = _Tally("analytic mean %s %s" % (mean, kernel))
    for D in [5] + dc.D_EDGES:
        c, refs = _reference(dc.N_TILES, D, kernel, True, mean)
        mo = _model(c, D, mean)
        ctx = "n=%d D=%d %s mean=%s" % (dc.N_TILES, D, kernel, mean)
        _check_fit(tally, mo, c, refs, D, ctx)
        mo.fit(c.thetas)
        _check_predict(tally, mo, c, refs, D, ctx, deriv=False)
    tally.finish()


@pytest.mark.parametrize("kernel", dc.PER_DIM)
def test_pivoted_nugget_with_a_repeated_point(kernel):
    """nugget="pivot", n = 60 with the last design point a copy of the first: grad_lowrank_kernel, whose chunks of eight parameters end in
    one that holds only the covariance-scale term at D = 8, 16 and 80.  The fuzz's rules for repeats: cond over the accepted pivots, and
    (n <= 64) objective, gradient and mean are compared; nothing of the skipped block is."""
    tally = _Tally("pivot %s" % kernel)
    for D in (7, 8, 9, 16, 17, 80):
        c, refs = _reference(60, D, kernel, False, repeat=True)
        mo = _model(c, D)
        ctx = "pivot n=60 D=%d %s" % (D, kernel)
        print("%s: cond over the accepted pivots %s" % (ctx, ", ".join("%.3g" % r["cond"] for r in refs)))
        assert all(r["cond"] <= 1e11 for r in refs), ctx
        _check_fit(tally, mo, c, refs, D, ctx)
        mo.fit(c.thetas)
        for m in dc.M_TEST:
            mean = mo.predict(c.Xs[:m], deriv=False)[0]
            for k in range(E):
                tally.check("mean", mean[k], refs[k]["mean"][:m], D, "%s m=%d emulator %d" % (ctx, m, k), refs[k]["amp"])
    tally.finish()


@NUGGETS
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52"])
def test_hessian(kernel, fit):
    """plane groups of 2 (D = 2), 4 + a padded group (5, 6, 33) and 20 whole groups (80); the cases, the restatement and the bar -- 100 x the
    float64 / long double disagreement of the restatement -- are those of test_gpu_hessian.py"""
    from test_gpu_hessian import _case, _close, _gp
    for D in (2, 5, 6, 33, 80):
        X, t, theta, pri, H, bar = _case(33, D, kernel, fit)
        got = M.logpost_hessian(_gp(X, t, kernel, fit, pri), theta)
        assert got.shape == (theta.size, theta.size) and np.array_equal(got, got.T)
        _close(got, H, bar, "sweep hessian n=33 D=%d %s %s" % (D, kernel, "fit" if fit else "fixed"))


KERNEL_CLASSES = {"SquaredExponential": "SquaredExponentialKernel", "Matern52": "Matern52Kernel", "ProductMat52": "ProductMat52Kernel",
                  "UniformSqExp": "UniformSqExpKernel", "UniformMat52": "UniformMat52Kernel"}


@pytest.mark.parametrize("kernel", dc.KERNELS)
def test_kernel_objects(kernel):
    """kernel_f, kernel_deriv and kernel_inputderiv of the native kernel objects (kernel_object_kernel) for 5 x 70 points, at the bars of
    test_gpu_parity.py::test_kernel_objects_vs_reference_golden (test_cpu_only_kernel_objects_vs_reference_golden for the product and the
    uniform kernels); the oracle has the analytic input derivative of every kernel"""
    from mogp_emulator_amd import libgpgpu
    kern = getattr(libgpgpu, KERNEL_CLASSES[kernel])()
    first = kernel in ("SquaredExponential", "Matern52")
    for D in (17, 33, 80):
        rng = np.random.default_rng([5, D])
        x1, x2 = rng.random((5, D)) * dc.column_scale(D), rng.random((70, D)) * dc.column_scale(D)
        nc = dc.n_corr(kernel, D)
        params = dc.theta_of(D, kernel, False)
        theta, s2 = params[:nc], np.exp(params[nc])
        K = kern.kernel_f(x1, x2, params)
        dK = kern.kernel_deriv(x1, x2, params).reshape(nc + 1, 5, 70)
        dX = np.transpose(kern.kernel_inputderiv(x1, x2, params).reshape(70, 5, D), (2, 1, 0))
        wK, wdK, wdX = s2 * R.kernel_f(x1, x2, theta, kernel), s2 * R.kernel_deriv(x1, x2, theta, kernel), s2 * R.kernel_inputderiv(x1, x2, theta, kernel)
        print("sweep kernel object %s D=%d: relative differences K %.3g, dK/dtheta %.3g of max, dK/dx %.3g of max" % (
            kernel, D, np.max(np.abs(K / wK - 1.)), np.max(np.abs(dK[:nc] - wdK)) / np.max(np.abs(wdK)), np.max(np.abs(dX - wdX)) / np.max(np.abs(wdX))))
        assert K.shape == (5, 70)
        assert_allclose(K, wK, rtol=1e-13 if first else 1e-12)
        assert_allclose(dK[:nc], wdK, rtol=1e-12 if first else 1e-11, atol=1e-15 if first else 1e-14)
        assert_allclose(dK[nc], K, rtol=1e-14)
        assert_allclose(dX, wdX, rtol=1e-11, atol=1e-14)


# ---- callers that reach the cross covariance with other views (a slot index, no K* output), one case each at D = 33 ------------------------

def test_leave_one_out_at_D_33():
    """cross_validate against cv_restate.fast, at the bars of test_gpu_cv.py (100 x the restatement's float64 / long double disagreement)"""
    import cv_restate as cr
    from test_gpu_cv import _bars, _close, _gp
    c = dc.case(dc.N_TILES, 33, "Matern52")
    X, t, theta, labels = c.X, c.T[0], c.thetas[0], np.arange(dc.N_TILES)
    a = cr.fast(X, t, theta, labels, dc.N_TILES, c.kernel, "zero", False, dc.NUGGET)
    b = cr.fast(X, t, theta, labels, dc.N_TILES, c.kernel, "zero", False, dc.NUGGET, dtype=np.longdouble)
    bars = _bars(a, b, "sweep loo D=33")
    gp = _gp(X, t, c.kernel, dc.NUGGET)
    gp.fit(theta)
    _close(M.cross_validate(gp), a, bars, "sweep loo D=33")


def test_sample_posterior_at_D_33():
    """the moments sample_posterior draws around are those of predict(full_cov=True), bit for bit, and the oracle's at the fuzz's bars; the
    draws are sample_restate's from these moments, at the bar of test_gpu_sample.py"""
    import sample_restate as sr
    from test_gpu_sample import _draw_bar
    D, m, S = 33, 65, 3
    tally = _Tally("sample")
    c, refs = _reference(dc.N_TILES, D, "SquaredExponential", True)
    mo = _model(c, D)
    mo.fit(c.thetas)
    p = mo.predict(c.Xs, full_cov=True, include_nugget=False, deriv=False)
    nug = mo._nuggets()
    z = np.random.default_rng(33).standard_normal((E, S, m))
    r = M.sample_posterior(mo, c.Xs, z=z)
    assert r.ok.all() and np.array_equal(r.mean, p.mean)
    worst = 0.
    for k in range(E):
        tally.check("mean", r.mean[k], refs[k]["mean"], D, "sample emulator %d" % k)
        want = R.GPRef(c.X, c.T[k], kernel=c.kernel, nugget="fit")
        want.fit(c.thetas[k])
        tally.check("fullcov", p.unc[k], want.predict(c.Xs, full_cov=True, include_nugget=False)[1], D, "sample emulator %d" % k)
        ref, ju, ok, St = sr.sample(p.mean[k], p.unc[k], z[k], nugget=nug[k])
        assert ok and ju == 0.
        bar = _draw_bar(St, z[k])
        err = np.max(np.abs(r.samples[k] - ref), axis=-1)
        print("sweep sample D=33 emulator %d: cond %.3g, device vs restatement at most %.3g, at most %.3g of the bar" % (
            k, np.linalg.cond(St), err.max(), np.max(err / bar)))
        worst = max(worst, float(np.max(err / bar)))
    tally.finish()
    assert worst <= 1.


def test_mixture_prediction_at_D_33():
    """predict_mixture over five samples of theta against marginal_restate.mixture, at the bars of test_gpu_marginal.py"""
    from test_gpu_marginal import _close, _gp, _reference as reference, _weights
    c = dc.case(dc.N_TILES, 33, "SquaredExponential")
    X, t, Xs = c.X, c.T[0], c.Xs
    thetas = c.thetas[0] + 0.15 * np.random.default_rng(3).standard_normal((5, c.thetas.shape[1]))
    w = _weights("nonuniform", 5)
    ref, bars = reference(X, t, thetas, Xs, c.kernel, "zero", False, dc.NUGGET, w, None, True, "sweep mixture D=33")
    gp = _gp(X, t, c.kernel, dc.NUGGET)
    gp.fit(thetas[0])
    got = gp._densegp_gpu.predict_mixture(thetas, Xs, weights=w, include_nugget=True)
    assert got[0].shape == (Xs.shape[0],) and got[5].all()
    _close(got, ref, bars, "sweep mixture D=33")
