"""Times of local approximate GP prediction (mogp_emulator_amd.LocalGP) on one MI355X, median of --reps (after one warm-up), as JSON lines:

 large     N design points in D dimensions, k neighbours, m queries (default N = 10^5, D = 10, k = 64, m = 10^4, then N = 10^6 where the
           device has room): the whole ``predict`` call, and from the HIP-event times of its two kernels
             local_knn   the time and the achieved fp64 vector rate against 3 m N D flops;
             local_gp    the time per query per workgroup (kernel time x resident workgroups / m; one workgroup is resident per compute
                         unit, 256 of them), to set beside the 27.3 us of one stand-alone 128 x 128 factorisation on one workgroup
                         (csrc/chol128_dev.h): the floor of that figure;
           against the host restatement -- brute-force NumPy distances, np.lexsort, LAPACK Cholesky and two triangular solves per query, on
           the threads the process is given -- run on --host-queries of the queries and SCALED UP to m (said so in the output), with the
           largest difference of the two on those queries.
 accuracy  N = 16000 (the size of the largest dense configuration), D = 10: the RMSE of the local mean against the dense ``predict`` at the
           same hyperparameters, relative to the spread of the targets, for k = 32, 64, 126.

    python tests/tools/local_timing.py [--N 100000] [--D 10] [--k 64] [--m 10000] [--reps 5] [--host-queries 200] [--limit 600]

Every step is a child process under its own ``timeout``; a step that fails, or runs out of time, ends the run (nothing further is started
on the device).  Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHOL128_STANDALONE_US = 27.3          # csrc/chol128_dev.h


def median_time(fn, reps, warm=True):
    if warm:
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, out


def kernel_ms(lib, fn, tags):
    lib.mogp_profile_reset()
    lib.mogp_profile_enable(1)
    fn()
    lib.mogp_profile_enable(0)
    out = {}
    for tag in tags:
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0 and ms.value > 0:
            out[tag] = {"ms": ms.value, "launches": cnt.value, "tflops": fl.value / ms.value * 1e-9}
    return out


def data(N, D, m, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.random((N, D))
    w = rng.normal(size=D)
    t = np.sin(X @ w) + 0.3 * X[:, 0] ** 2 + 0.05 * rng.standard_normal(N)
    return X, t, rng.random((m, D))


def fitted(X, t, D, n_sub):
    """the emulator the hyperparameters come from: fitted at a fixed theta on the first n_sub rows"""
    import mogp_emulator_amd as M
    from mogp_emulator_amd.Priors import GPPriors
    theta = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -6.]])
    gp = M.GaussianProcessGPU(X[:n_sub], t[:n_sub], nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
    gp.fit(theta)
    return gp, theta


def host_restatement(X, t, Q, s, sigma2, nugget, k):
    """brute-force NumPy neighbours (local_restate.neighbours), then LAPACK Cholesky and two triangular solves per query"""
    import local_restate as lr
    from scipy.linalg import solve_triangular
    nbr, radius, _ = lr.neighbours(X, Q, s, k)
    mean, var = np.empty(Q.shape[0]), np.empty(Q.shape[0])
    Xt, Qt = X * s, Q * s
    for j in range(Q.shape[0]):
        P = Xt[nbr[j]]
        d2 = np.sum((P[:, None, :] - P[None, :, :]) ** 2, axis=-1)
        Kq = sigma2 * np.exp(-0.5 * d2) + nugget * np.eye(k)
        ks = sigma2 * np.exp(-0.5 * np.sum((P - Qt[j]) ** 2, axis=-1))
        L = np.linalg.cholesky(Kq)
        z = solve_triangular(L, np.stack([t[nbr[j]], ks], axis=1), lower=True)
        mean[j] = z[:, 0] @ z[:, 1]
        var[j] = max(sigma2 - z[:, 1] @ z[:, 1] + nugget, 0.)
    return nbr, mean, var


def step_large(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    import local_restate as lr
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, k, m = args.N, args.D, args.k, args.m
    X, t, Q = data(N, D, m)
    gp, theta = fitted(X, t, D, 2000)
    t0 = time.perf_counter()
    lg = M.LocalGP(gp, X, t, n_neighbours=k)
    create_s = time.perf_counter() - t0
    call = lambda: lg.predict(Q)                                          # noqa: E731
    t_c, all_c, res = median_time(call, args.reps)
    kern = kernel_ms(lib, call, ("local_knn", "local_gp"))
    resident = min(m, 256)           # the kernel's registers admit one workgroup per compute unit, 256 compute units
    out = {"step": "large", "N": N, "D": D, "k": k, "m": m, "create_s": create_s, "predict_s": t_c, "predict_all_s": all_c,
           "n_failed": res.n_failed, "kernels": kern}
    if "local_knn" in kern:
        out["knn_fp64_vector_tflops"] = 3. * m * N * D / (kern["local_knn"]["ms"] * 1e-3) * 1e-12
    if "local_gp" in kern:
        out["gp_us_per_query_per_workgroup"] = kern["local_gp"]["ms"] * 1e3 * resident / m
        out["gp_resident_workgroups_assumed"] = resident
        out["chol128_standalone_us"] = CHOL128_STANDALONE_US
    # the host restatement on a subset of the queries, scaled up
    hq = max(1, min(args.host_queries, m, max(10, 20000000 // N)))       # the (queries, N) distance matrix stays in the hundreds of MB
    s = lr.scales(theta[:D], D, "SquaredExponential")
    sigma2, nugget = float(np.exp(theta[D])), float(gp.nugget)

    t_h, all_h, (nbr, mean, var) = median_time(lambda: host_restatement(X, t, Q[:hq], s, sigma2, nugget, k), 1, warm=False)
    sub = lg.predict(Q[:hq], return_neighbours=True)
    out.update({"host_queries": hq, "host_subset_s": t_h, "host_scaled_to_m_s": t_h * m / hq, "host_scaled_ratio": t_h * m / hq / t_c,
                "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"), "neighbours_equal_on_subset": bool(np.array_equal(sub.neighbours, nbr)),
                "max_abs_diff_mean": float(np.max(np.abs(sub.mean - mean))), "max_abs_diff_var": float(np.max(np.abs(sub.unc - var)))})
    lg.close()
    print(json.dumps(out))


def step_accuracy(args):
    import mogp_emulator_amd as M
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D, m = 16000, args.D, 2000
    X, t, Q = data(N, D, m, seed=2)
    gp, theta = fitted(X, t, D, N)
    dense = gp.predict(Q, deriv=False)
    out = {"step": "accuracy", "N": N, "D": D, "m": m, "target_std": float(np.std(t))}
    for k in (32, 64, 126):
        p = M.predict_local(gp, X, t, Q, n_neighbours=k)
        out["k%d" % k] = {"rmse_over_target_std": float(np.sqrt(np.mean((p.mean - dense.mean) ** 2)) / np.std(t)), "n_failed": p.n_failed,
                          "mean_unc_ratio": float(np.mean(p.unc) / np.mean(dense.unc))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-queries", type=int, default=200)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["large", "accuracy"], default=None)
    args = ap.parse_args()
    if args.step == "large":
        return step_large(args)
    if args.step == "accuracy":
        return step_accuracy(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--k", str(args.k), "--m", str(args.m),
            "--reps", str(args.reps), "--host-queries", str(args.host_queries)]
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
