"""The iterative exact likelihood on the MI355X (IterativeGP.log_likelihood, VecchiaGP.loglik_exact / fit_exact; csrc/kernels_iter.hip
kgrad_forms_kernel and probe_kernel, csrc/engine_iter_lik.hip) against the NumPy restatement (exact_lik_restate.py), at the smallest shapes where
the code can go another way: designs of two to five row tiles with a partial last one, one to five slices of 16 dimensions, 1 / 15 / 16 / 31
probes (one, four, five and eight MFMA steps; one and two blocks of 16 columns in the product), every kernel, a preconditioner that stops
early and none at all.  test_exact_lik_host.py shows on the CPU that the restatement is right and that float64 lies inside the forms' bar.
Measured figures are printed as fractions of their bars; DESIGN.md section 3 "Iterative exact likelihood" records them."""
import numpy as np
import pytest

import mogp_emulator_amd as M

import dimension_cases as dc
import exact_lik_restate as er
import iterative_restate as ir
import test_exact_lik_host as eh
import test_gpu_iterative as tg
import test_iterative_host as th
import vecchia_cases as vc
from test_iterative_host import MAX_ITER, RTOL, SIGMA2

pytestmark = pytest.mark.gpu

ETA = dc.NUGGET
FORMS_CASES = ([(N, 3, 15, k, 32) for N in (126, 130, 300) for k in th.FOUR] +
               [(130, D, 15, k, 32) for D in (1, 17, 80) for k in th.FOUR] +
               [(130, 3, T, k, 32) for T in (1, 16, 31) for k in th.FOUR])


def _pieces(ig, g1, g2, p, rtol=RTOL, max_iter=MAX_ITER, **kw):
    kt, s, sigma2, eta = ig._hyper[0][:4]
    return ig._native.loglik_exact(0, kt, s, sigma2, eta, p, rtol, max_iter, g1, g2, **kw)


def _quadrature(r, t):
    """e_1^T log(T) e_1 of probe t from the device's coefficient log, by the package's own rule"""
    m = r["iterations"][1 + t]
    return eh.IG._lanczos_quadrature(r["coef"][:m, 0, 1 + t], r["coef"][:m, 1, 1 + t])


def _rank(ig, p):
    kt, s, sigma2, eta = ig._hyper[0][:4]
    return ig._native.precondition(kt, s, sigma2, eta, p)[0]


def _group_fractions(c, s, kernel, r):
    """(fraction of the bar of the data group, of the probe group) per dimension, of the pieces r with their own panels"""
    U, W = r["x"], r["w"]
    truth = er.forms(c.X, s, kernel, SIGMA2, U, W)
    bar = er.forms_bar(c.X, s, kernel, SIGMA2, U, W)
    f64 = er.forms(c.X, s, kernel, SIGMA2, U, W, dtype=np.float64)
    fr = lambda got, cols: np.abs(np.asarray(got.astype(np.longdouble) - truth[:, cols].sum(axis=1), dtype=np.float64)) / bar[:, cols].sum(axis=1)
    probe = slice(1, U.shape[1])
    host = max(fr(f64[:, 0], slice(0, 1)).max(), fr(f64[:, probe].sum(axis=1), probe).max())
    return fr(r["forms_data"], slice(0, 1)), fr(r["forms_probe"], probe), host, bar


# ---- 1. the sweep ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,T,kernel,p", FORMS_CASES, ids=lambda v: str(v))
def test_kgrad_forms_against_the_long_double_restatement(N, D, T, kernel, p):
    c, s, ig = tg._iter(N, D, kernel, p, rtol=1e-6)
    rank = _rank(ig, p)
    g1, g2 = eh.caller_probes(N, rank, T)
    r = _pieces(ig, g1, g2, p, rtol=1e-6, grad=True, return_panels=True)
    again = _pieces(ig, g1, g2, p, rtol=1e-6, grad=True)
    h1, h2 = eh.caller_probes(N, rank, T, seed=3)
    other = _pieces(ig, h1, h2, p, rtol=1e-6, grad=True)
    if kernel in ir.UNIFORM:                      # the one parameter of a uniform kernel: the D forms added in ascending d, bit for bit
        view = M.IterativeGP._on_handle(ig._native, ig._hyper, D, N, precond_rank=p, rtol=1e-6, max_iter=MAX_ITER, layout=[(True, False)])
        ll = view.log_likelihood(grad=True, probes=(g1, g2))
        tot_d, tot_p = 0., 0.
        for d in range(D):
            tot_d, tot_p = tot_d + r["forms_data"][d], tot_p + r["forms_probe"][d]
        assert ll.trace.shape == (2,) and ll.data_forms[0] == tot_d and ll.trace[0] == tot_p / T
    ig.close()
    assert r["converged"].all() and r["forms_data"].shape == r["forms_probe"].shape == (D,)
    assert np.array_equal(r["forms_data"], again["forms_data"]) and np.array_equal(r["forms_probe"], again["forms_probe"])
    assert np.array_equal(r["forms_data"], other["forms_data"]) and not np.array_equal(r["forms_probe"], other["forms_probe"])
    fd, fp, host, _ = _group_fractions(c, s, kernel, r)
    print("N %d D %d T %d %s: data forms at %.3g, probe forms at %.3g of the bar (float64 restatement %.3g)" % (N, D, T, kernel, fd.max(), fp.max(), host))
    assert 0. < host <= 1.
    assert fd.max() < 1. and fp.max() < 1.


# ---- 2. the probes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,kernel,p", [(300, 3, "SquaredExponential", 64), (130, 1, "SquaredExponential", 32), (130, 3, "Matern52", 0)], ids=lambda v: str(v))
def test_probes_against_the_restatement_on_the_devices_factor(n, D, kernel, p):
    c, s, ig = tg._iter(n, D, kernel, p, rtol=1e-6)
    L = ig.preconditioner()[0] if p else np.zeros((n, 0))
    r = L.shape[1]
    g1, g2 = eh.caller_probes(n, r, 15)
    z = _pieces(ig, g1, g2, p, rtol=1e-6, return_panels=True)["z"]
    ig.close()
    root = np.sqrt(ETA) if r else 1.
    L80, g180, g280 = L.astype(np.longdouble), g1.astype(np.longdouble), g2.astype(np.longdouble)
    truth = L80 @ g180 + np.longdouble(root) * g280
    bar = 2. ** -52 * (r + 4) * (np.abs(L) @ np.abs(g1) + root * np.abs(g2))          # a fixed-order sum of r + 1 products
    frac = tg._fraction_of_bar(z, truth, bar)
    print("n %d D %d %s p %d: rank %d, probes at %.3g of their bar" % (n, D, kernel, p, r, frac))
    assert frac <= 1.
    if r == 0:
        assert np.array_equal(z, g2)


# ---- 3. logging changes nothing --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [64, 0])
def test_the_coefficient_log_changes_no_bit_of_the_solve(p):
    n, D, kernel = 300, 3, "SquaredExponential"
    c, s, ig = tg._iter(n, D, kernel, p)
    g1, g2 = eh.caller_probes(n, _rank(ig, p), 7)
    r = _pieces(ig, g1, g2, p, return_panels=True)
    sv = ig.solve(np.column_stack([c.T[0], r["z"]]))
    alpha = ig.weights()
    ig.close()
    print("p %d: iterations %s" % (p, r["iterations"].tolist()))
    assert np.array_equal(sv.x, r["x"]) and np.array_equal(sv.iterations, r["iterations"]) and np.array_equal(sv.residual, r["residual"])
    assert np.array_equal(sv.converged, r["converged"]) and sv.converged.all()
    assert np.array_equal(alpha, r["x"][:, 0])                  # the kept alpha is the one predict would solve
    # the log holds exactly `iterations` alphas and one beta fewer per column, positive, and nothing behind them
    for col, m in enumerate(r["iterations"]):
        a, b = r["coef"][:, 0, col], r["coef"][:, 1, col]
        assert np.all(a[:m] > 0.) and np.all(b[:m - 1] > 0.) and not a[m:].any() and not b[m - 1:].any()


# ---- 4. the estimator with the caller's probes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,p", [(300, 3, 64), (1000, 5, 256)], ids=lambda v: str(v))
@pytest.mark.parametrize("kernel", ["SquaredExponential", "Matern52", "UniformSqExp"])
def test_estimator_with_the_callers_probes(n, D, p, kernel):
    T = 15
    c, s, ig = tg._iter(n, D, kernel, p)
    L = ig.preconditioner()[0]
    g1, g2 = eh.caller_probes(n, L.shape[1], T)
    r = _pieces(ig, g1, g2, p, grad=True, return_panels=True)
    ll = ig.log_likelihood(grad=True, probes=(g1, g2))
    ig.close()
    y = c.T[0]
    ref = er.estimator_dense(c.X, y, s, kernel, SIGMA2, ETA, L, g1, g2)
    host = er.estimator_pcg(c.X, y, s, kernel, SIGMA2, ETA, L, g1, g2, RTOL, MAX_ITER)
    assert r["converged"].all() and host["converged"].all() and ll.ok
    print("n %d D %d %s p %d: iterations device %s host %s" % (n, D, kernel, p, r["iterations"].tolist(), host["iterations"].tolist()))
    quad_dev = r["rho"] * np.array([_quadrature(r, t) for t in range(T)])
    bar = er.forms_bar(c.X, s, kernel, SIGMA2, r["x"], r["w"])
    dot_bar = lambda a, b: 2. ** -52 * (n + 4) * np.sum(np.abs(a) * np.abs(b), axis=0)
    bar_rho, bar_uw = dot_bar(ref["z"], ref["w"]), dot_bar(ref["u"], ref["w"])
    worst = {}

    def check(name, dev, hst, want, kernel_bar):
        # the gap of a quantity is its largest over the probes / dimensions: per entry it is a matter of chance (both the host's and the
        # device's distance are mostly the dense reference's own error, of one size for all entries and of either sign)
        gap = np.max(np.abs(hst - want))
        allowed = 4. * gap + kernel_bar
        dist = np.abs(dev - want)
        worst[name] = (float(np.max(dist / allowed)), float(np.max(gap)), float(np.max(dist)))
        return allowed

    a_rho = check("rho", r["rho"], host["rho"], ref["rho"], bar_rho)
    a_uw = check("uw", r["uw"], host["uw"], ref["uw"], bar_uw)
    a_quad = check("quadrature", quad_dev, host["quad"], ref["quad"], bar_rho * np.abs(ref["quad"] / ref["rho"]))
    a_ya = check("y^T alpha", r["y_alpha"], host["y_alpha"], ref["y_alpha"], dot_bar(y, ref["alpha"]))
    a_aa = check("alpha^T alpha", r["alpha_alpha"], host["alpha_alpha"], ref["alpha_alpha"], dot_bar(ref["alpha"], ref["alpha"]))
    a_fd = check("data forms", r["forms_data"], host["forms_data"], ref["forms_data"], bar[:, 0])
    a_fp = check("probe forms", r["forms_probe"], host["forms_each"].sum(axis=0), ref["forms_each"].sum(axis=0), bar[:, 1:].sum(axis=1))
    # value and gradient: the same linear combinations of the pieces, and of what each piece is allowed
    want = er.assemble(ref, n, ETA, kernel, fit_nugget=False)
    a_value = 0.5 * a_ya + 0.5 * np.mean(a_quad)
    corr = (lambda v: np.array([v.sum()])) if kernel in ir.UNIFORM else (lambda v: v)
    a_grad = np.concatenate([0.5 * corr(a_fd) + 0.5 * corr(a_fp) / T, [0.5 * (a_ya + ETA * a_aa) + 0.5 * (np.mean(a_rho) + ETA * np.mean(a_uw))]])
    worst["value"] = (abs(ll.value - want["value"]) / a_value, 0., abs(ll.value - want["value"]))
    worst["grad"] = (float(np.max(np.abs(ll.grad - want["grad"]) / a_grad)), 0., float(np.max(np.abs(ll.grad - want["grad"]))))
    for name, (frac, gap, dist) in worst.items():
        print("  %-14s device at %.3g of what it is allowed (host gap %.3g, device distance %.3g)" % (name, frac, gap, dist))
    assert ll.grad.shape == want["grad"].shape
    assert all(frac <= 1. for frac, _, _ in worst.values()), worst


# ---- 5. the Vecchia identity ---------------------------------------------------------------------------------------------------------------------
def test_exact_likelihood_is_vecchias_at_k_equal_to_n_minus_1():
    N, D, k = vc.LIMIT
    kernel, rtol = "SquaredExponential", 1e-10
    c, theta, s, sigma2, nugget = vc.setup(N, D, kernel, True)
    y = c.T[0]
    vg = M.VecchiaGP(c.X, y, kernel=kernel, n_neighbours=k, nugget="fit", order=np.arange(N))
    vg.set_neighbours(theta=theta)
    v = vg.loglik(theta, grad=True)
    ll = vg.loglik_exact(theta, grad=True, n_probes=31, seed=eh.VECCHIA_SEED, precond_rank=eh.VECCHIA_RANK, rtol=rtol, probe_terms=True)
    vg.close()
    want = er.dense_loglik(c.X, y, s, kernel, sigma2, nugget)
    A = ir.operator(c.X, s, kernel, sigma2, nugget)
    cond = np.linalg.cond(A)
    tol = cond * (rtol + N * 2. ** -52)                          # |alpha - A^-1 y| <= cond rtol |alpha|, and what the dense values are off by
    na, ny = np.linalg.norm(want["alpha"]), np.linalg.norm(y)
    fit_implied = -2. * (v.value + 0.5 * N * np.log(2. * np.pi)) - want["logdet"]
    data_implied = 2. * v.grad + want["traces"]
    dA = er.derivative_matrices(c.X, s, kernel, sigma2, nugget)
    scale = np.array([2. * na * na * np.linalg.norm(Mq, 2) for Mq in dA])
    print("fit term %.10g against %.10g; data forms off by %s of their tolerance" %
          (ll.fit_term, fit_implied, np.round(np.abs(ll.data_forms - data_implied) / (tol * scale), 4).tolist()))
    assert ll.ok and abs(ll.fit_term - fit_implied) <= tol * ny * na
    assert np.all(np.abs(ll.data_forms - data_implied) <= tol * scale)
    zs = np.concatenate([[(ll.logdet - want["logdet"]) / ll.logdet_se], (ll.trace - want["traces"]) / ll.trace_se])
    print("z-scores of the log-determinant and the traces: %s" % np.round(zs, 2).tolist())
    assert np.all(np.abs(zs) <= 4.)


# ---- 6 - 8, 10 ---------------------------------------------------------------------------------------------------------------------------------------
def test_early_stop_sizes_g1_by_the_rank_reached():
    c, s, ig = tg._iter(130, 1, "SquaredExponential", 32)
    ll = ig.log_likelihood(grad=True)
    rank = len(ig.preconditioner()[1])
    with pytest.raises(ValueError, match="as many rows as the rank the preconditioner reaches, %d" % rank):
        ig.log_likelihood(probes=eh.caller_probes(130, 32, 3))
    ig.close()
    assert ll.precond_rank == rank < 32 and ll.ok and np.isfinite(ll.value) and np.all(np.isfinite(ll.grad))


def test_nugget_and_variance_traces_are_the_returned_scalars_bit_for_bit():
    for kernel, p in (("Matern52", 64), ("UniformSqExp", 0)):
        c, s, ig = tg._iter(300, 3, kernel, p)
        view = M.IterativeGP._on_handle(ig._native, ig._hyper, 3, 300, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER,
                                        layout=[(kernel in ir.UNIFORM, True)])       # with the nugget's entry in the layout
        ll = view.log_likelihood(grad=True, n_probes=7)
        ig.close()
        assert ll.ok and ll.trace.shape == (dc.n_corr(kernel, 3) + 2,)
        assert ll.trace[-1] == ETA * np.mean(ll.uw) and ll.trace[-2] == np.mean(ll.rho) - ETA * np.mean(ll.uw)
        assert np.all(np.isfinite(ll.trace_se[-2:])) and np.all(np.isnan(ll.trace_se[:-2]))


def test_a_run_that_cannot_converge_is_reported_not_raised():
    c, s, ig = tg._iter(300, 3, "SquaredExponential", 0, max_iter=5)
    ll = ig.log_likelihood(grad=True)
    ig.close()
    assert not ll.ok and np.isnan(ll.value) and np.all(np.isnan(ll.grad)) and not ll.converged.all()
    assert np.all(ll.iterations == 5) and np.all(ll.residual > RTOL)


def test_probe_terms_give_the_grouped_sweep_and_a_standard_error():
    n, D, kernel, p, T = 130, 3, "SquaredExponential", 32, 15
    c, s, ig = tg._iter(n, D, kernel, p)
    g1, g2 = eh.caller_probes(n, _rank(ig, p), T)
    r = _pieces(ig, g1, g2, p, grad=True, probe_terms=True, return_panels=True)
    ll = ig.log_likelihood(grad=True, probes=(g1, g2), probe_terms=True)
    ig.close()
    bar = er.forms_bar(c.X, s, kernel, SIGMA2, r["x"], r["w"])[:, 1:].sum(axis=1)
    frac = np.abs(r["forms_each"].sum(axis=0) - r["forms_probe"]) / bar                # the bar of test 1 of the probe group
    print("per-probe sweeps against the grouped sweep: %.3g of the bar" % frac.max())
    assert frac.max() <= 1. and np.all(np.isfinite(ll.trace_se)) and np.all(ll.trace_se > 0.)
    assert np.array_equal(ll.trace[:D], r["forms_probe"] / T)


# ---- 9. the fit ---------------------------------------------------------------------------------------------------------------------------------------
def test_fit_exact_climbs_the_dense_likelihood():
    X, y, theta_true, start = eh.fit_problem()
    vg = M.VecchiaGP(X, y, kernel=eh.FIT_KERNEL, n_neighbours=30, nugget="fit", order=np.arange(X.shape[0]))
    fit = vg.fit_exact(theta0=start, n_probes=eh.FIT_PROBES, seed=eh.FIT_SEED, precond_rank=eh.FIT_RANK, rtol=eh.FIT_RTOL)
    assert np.array_equal(vg.theta, fit.theta)
    vg.close()
    print("%d evaluations, %s" % (fit.n_evaluations, fit.message))
    assert isinstance(fit, M.ExactFit) and fit.loglik.ok and fit.value == fit.loglik.value
    eh.check_fit(X, y, start, fit.theta, fit.converged)
