"""Times of the Vecchia likelihood (mogp_emulator_amd.VecchiaGP) on one MI355X, median of --reps (after one warm-up), as JSON lines:

 large     N design points in D dimensions, k neighbours (default N = 10^5, D = 10, k = 30, then N = 10^6 where the device has room), random
           order, squared exponential, nugget fitted, at a fixed theta:
             set_neighbours          the whole call, and the HIP-event time of the ordered search with its fp64 vector rate against
                                     1.5 N^2 D flops (half of the N x N sweep);
             loglik                  without and with the gradient: the whole call, the HIP-event time of the kernel, and that time per
                                     point per resident workgroup (kernel time x 256 / N: one workgroup is resident per compute unit), to
                                     set beside local_gp's 35 us and the 27.3 us of one stand-alone 128 x 128 factorisation;
             fit                     one whole ``fit(theta0, refresh=2)`` with its number of evaluations;
           against the NumPy restatement (vecchia_restate.py: brute-force distances over the prefix, np.lexsort, its own Cholesky, the
           analytic gradient) run on --host-points of the points, evenly spaced through the order so that their prefixes average N / 2, and
           SCALED UP to N (said so in the output), with the largest difference of the terms on those points.
 accuracy  N = 16000, D = 10, 2000 queries -- the targets and the dense reference of local_timing.py's accuracy step (the dense ``predict``
           at that step's fixed theta on all 16000 points): the RMSE of the ``LocalGP`` mean, relative to the spread of the targets, with
           theta from ``VecchiaGP.fit`` on ALL points and with theta from the dense MAP fit of a 2000-point subsample, for k = 32, 64, 126.

    python tests/tools/vecchia_timing.py [--N 100000] [--D 10] [--k 30] [--reps 3] [--host-points 100] [--limit 900]

Every step is a child process under its own ``timeout``; a step that fails, or runs out of time, ends the run (nothing further is started
on the device).  Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import local_timing as lt          # noqa: E402  (data, median_time, kernel_ms and the fixed theta of its steps)

RESIDENT = 256                      # the kernel's registers admit one workgroup per compute unit, 256 compute units


def fixed_theta(D):
    return np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -6.]])


def step_large(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    import local_restate as lr
    import vecchia_restate as vr
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, k = args.N, args.D, args.k
    X, t, _ = lt.data(N, D, 1)
    theta = fixed_theta(D)
    t0 = time.perf_counter()
    vg = M.VecchiaGP(X, t, n_neighbours=k, rng=0)
    create_s = time.perf_counter() - t0
    out = {"step": "large", "N": N, "D": D, "k": k, "create_s": create_s}
    search = lambda: vg.set_neighbours(theta=theta)                       # noqa: E731
    t_s, all_s, _ = lt.median_time(search, args.reps)
    kern = lt.kernel_ms(lib, search, ("vecchia_knn",))
    out.update({"set_neighbours_s": t_s, "set_neighbours_all_s": all_s, "kernels": kern})
    if "vecchia_knn" in kern:
        out["knn_fp64_vector_tflops"] = 1.5 * N * N * D / (kern["vecchia_knn"]["ms"] * 1e-3) * 1e-12
    for name, grad, tag in (("loglik", False, "vecchia_ll"), ("loglik_grad", True, "vecchia_ll_grad")):
        call = lambda: vg.loglik(theta, grad=grad)                        # noqa: E731
        t_c, all_c, res = lt.median_time(call, args.reps)
        kk = lt.kernel_ms(lib, call, (tag,))
        out.update({name + "_s": t_c, name + "_all_s": all_c, name + "_n_failed": res.n_failed, name + "_value": res.value})
        if tag in kk:
            out[name + "_kernel_ms"] = kk[tag]["ms"]
            out[name + "_us_per_point_per_workgroup"] = kk[tag]["ms"] * 1e3 * min(N, RESIDENT) / N
    t0 = time.perf_counter()
    fit = vg.fit(theta0=theta, refresh=2)
    out.update({"fit_s": time.perf_counter() - t0, "fit_evaluations": fit.n_evaluations, "fit_converged": fit.converged, "fit_value": fit.value,
                "fit_theta": fit.theta.tolist()})
    # the restatement on a subset of the points, scaled up
    vg.set_neighbours(theta=theta)
    dev = vg.loglik(theta, grad=True, return_terms=True)
    order = vg.order
    Xo, yo = X[order], t[order]
    hp = max(2, min(args.host_points, N))
    rows = np.unique(np.linspace(0, N - 1, hp).astype(int))
    s, sigma2, nugget = vr.unpack(theta, D, "SquaredExponential", "fit")

    def host():
        nbr = np.full((N, k), -1, dtype=np.int64)
        for p in rows:
            if p > 0:
                idx = np.lexsort((np.arange(p), lr.scaled_r2(Xo[:p], Xo[p:p + 1], s)[0]))[:k]
                nbr[p, :len(idx)] = idx
        return vr.terms(Xo, yo, s, "SquaredExponential", sigma2, nugget, nbr, grad=True, rows=rows)
    t0 = time.perf_counter()
    terms, g, ok, _ = host()
    t_h = time.perf_counter() - t0
    out.update({"host_points": int(len(rows)), "host_subset_s": t_h, "host_scaled_to_N_s": t_h * N / len(rows),
                "host_scaled_ratio_to_search_plus_gradient": t_h * N / len(rows) / (t_s + out["loglik_grad_s"]),
                "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
                "max_abs_diff_terms": float(np.max(np.abs(dev.terms[order][rows] - terms[rows])))})
    vg.close()
    print(json.dumps(out))


def step_accuracy(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D, m, n_sub = 16000, args.D, 2000, 2000
    X, t, Q = lt.data(N, D, m, seed=2)
    gp, theta = lt.fitted(X, t, D, N)
    dense = gp.predict(Q, deriv=False)
    spread = float(np.std(t))
    out = {"step": "accuracy", "N": N, "D": D, "m": m, "target_std": spread, "dense_theta": theta.tolist()}
    # theta from the dense MAP fit of a subsample
    sub = M.GaussianProcessGPU(X[:n_sub], t[:n_sub], nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
    t0 = time.perf_counter()
    sub = M.fit_GP_MAP(sub, n_tries=3)
    out["subsample_fit_s"] = time.perf_counter() - t0
    out["subsample_theta"] = np.asarray(sub.theta.get_data(), dtype=float).tolist()
    # theta from the Vecchia fit of all points
    vg = M.VecchiaGP(X, t, n_neighbours=args.k, rng=0)
    t0 = time.perf_counter()
    fit = vg.fit(refresh=2)
    out.update({"vecchia_fit_s": time.perf_counter() - t0, "vecchia_theta": fit.theta.tolist(), "vecchia_evaluations": fit.n_evaluations,
                "vecchia_converged": fit.converged})

    def rmse(mean):
        return float(np.sqrt(np.mean((mean - dense.mean) ** 2)) / spread)
    for k in (32, 64, 126):
        ps = M.predict_local(sub, X, t, Q, n_neighbours=k)
        pv = vg.predict(Q, n_neighbours=k)
        pd = M.predict_local(gp, X, t, Q, n_neighbours=k)
        out["k%d" % k] = {"rmse_theta_of_subsample_fit": rmse(ps.mean), "rmse_theta_of_vecchia_fit": rmse(pv.mean), "rmse_dense_theta": rmse(pd.mean),
                          "n_failed": [ps.n_failed, pv.n_failed, pd.n_failed]}
    vg.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=100)
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=["large", "accuracy"], default=None)
    args = ap.parse_args()
    if args.step == "large":
        return step_large(args)
    if args.step == "accuracy":
        return step_accuracy(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--k", str(args.k),
            "--reps", str(args.reps), "--host-points", str(args.host_points)]
    steps = [("large", ["--N", str(args.N)])]
    if args.N < 1000000:
        steps.append(("large", ["--N", "1000000"]))
    steps.append(("accuracy", []))
    for name, extra in steps:
        rc = subprocess.run(base + ["--step", name] + extra).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
