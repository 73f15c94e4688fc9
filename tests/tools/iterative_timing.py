"""Times of the iterative exact prediction (mogp_emulator_amd.IterativeGP) on one MI355X, as JSON lines.  Squared exponential, D = 10,
hyperparameters of an emulator fitted at a fixed theta on a 2000-point subsample (those of tests/tools/local_timing.py):

 large     N design points (default 10^5, then 16 000):
             kmatvec        the product with r = 1 / 16 / 32 right-hand sides: the kernel's HIP-event time (median of --reps) and the whole
                            call with its host copies; the expectation to hold it against is that the entries' generation binds, so that
                            32 right-hand sides cost little more than one
             precondition   the build of the rank-p pivoted Cholesky preconditioner, p = 64 / 256 / 1024 (rank reached, wall time)
             alpha          iterations, convergence, recomputed residual and wall time of the solve for the weights at p = 0 / 64 / 256 /
                            1024 (rtol 1e-8, at most 1000 iterations), the preconditioner already built
             mean           the mean at m = 10^4 queries (alpha kept), p = 256
             variance       the variance at 256 queries (eight solves of 32 cross columns), p = 256
 accuracy  N = 16 000, 2000 queries: the RMSE of this mean and of LocalGP's (k = 126) against the dense ``predict`` at the same
           hyperparameters, relative to the spread of the targets, and the ratio of the mean variances on the first 64 queries.

    python tests/tools/iterative_timing.py [--N 100000] [--D 10] [--m 10000] [--reps 3] [--limit 900]

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

RTOL, MAX_ITER = 1e-8, 1000


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


def kernel_ms(lib, fn, tag, reps):
    """median HIP-event time of the kernels filed under `tag` over `reps` calls of fn (after one warm-up)"""
    fn()
    out = []
    for _ in range(reps):
        lib.mogp_profile_reset()
        lib.mogp_profile_enable(1)
        fn()
        lib.mogp_profile_enable(0)
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0 and ms.value > 0:
            out.append(ms.value / max(1, cnt.value))
    return statistics.median(out) if out else None


def note(what, value):
    """progress on stderr: the JSON line of a step comes only at its end"""
    print(what, json.dumps(value), file=sys.stderr, flush=True)


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def step_large(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, m = args.N, args.D, args.m
    X, t, Q = data(N, D, m)
    gp, theta = fitted(X, t, D, 2000)
    out = {"step": "large", "N": N, "D": D, "rtol": RTOL, "max_iter": MAX_ITER, "nugget": float(gp.nugget)}
    ig = M.IterativeGP(gp, X, t, precond_rank=0, rtol=RTOL, max_iter=MAX_ITER)
    rng = np.random.default_rng(5)
    out["kmatvec"] = {}
    for r in (1, 16, 32):
        V = rng.standard_normal((N, r))
        call = lambda: ig.matvec(V)                                       # noqa: E731
        ms = kernel_ms(lib, call, "kmatvec", args.reps)
        out["kmatvec"]["r%d" % r] = {"kernel_ms": ms, "call_s": wall(call)[0], "entries_per_s": None if not ms else float(N) * N / (ms * 1e-3)}
        note("kmatvec r%d" % r, out["kmatvec"]["r%d" % r])
    ig.close()
    out["precondition"], out["alpha"] = {}, {}
    for p in (0, 64, 256, 1024):
        if p > N:
            continue
        ig = M.IterativeGP(gp, X, t, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        if p:
            s, (rank, _) = wall(lambda: ig._native.precondition(*ig._hyper[0][:4], p)[:2])
            out["precondition"]["p%d" % p] = {"build_s": s, "rank": int(rank)}
        s, sv = wall(lambda: ig.solve(t))
        out["alpha"]["p%d" % p] = {"solve_s": s, "iterations": int(sv.iterations[0]), "converged": bool(sv.converged[0]),
                                   "residual": float(sv.residual[0]), "rank": int(sv.precond_rank)}
        note("p%d" % p, [out["precondition"].get("p%d" % p), out["alpha"]["p%d" % p]])
        if p == 256:
            ig.weights()                                                  # alpha solved and kept: the mean below is the product alone
            s, pr = wall(lambda: ig.predict(Q))
            out["mean"] = {"m": m, "predict_s": s, "kernel_ms": kernel_ms(lib, lambda: ig.predict(Q), "kmatvec", 1)}
            s, pv = wall(lambda: ig.predict(Q[:256], unc=True))
            out["variance"] = {"m": 256, "predict_s": s, "converged": int(np.count_nonzero(pv.var_converged)),
                               "largest_residual": float(pv.var_residual.max())}
        ig.close()
    print(json.dumps(out))


def step_accuracy(args):
    import mogp_emulator_amd as M
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D, m = 16000, args.D, 2000
    X, t, Q = data(N, D, m, seed=2)
    gp, theta = fitted(X, t, D, N)
    dense = gp.predict(Q, deriv=False)
    sd = float(np.std(t))
    out = {"step": "accuracy", "N": N, "D": D, "m": m, "target_std": sd}
    p = M.predict_local(gp, X, t, Q, n_neighbours=126)
    out["local_k126"] = {"rmse_over_target_std": float(np.sqrt(np.mean((p.mean - dense.mean) ** 2)) / sd)}
    for rank in (256, 1024):
        ig = M.IterativeGP(gp, X, t, precond_rank=rank, rtol=RTOL, max_iter=MAX_ITER)
        s, pr = wall(lambda: ig.predict(Q))
        pv = ig.predict(Q[:64], unc=True)
        ig.close()
        out["iterative_p%d" % rank] = {"rmse_over_target_std": float(np.sqrt(np.mean((pr.mean - dense.mean) ** 2)) / sd), "predict_s": s,
                                       "iterations": int(pr.iterations), "converged": bool(pr.converged), "residual": float(pr.residual),
                                       "mean_unc_ratio_first_64": float(np.mean(pv.unc) / np.mean(dense.unc[:64])),
                                       "var_converged": int(np.count_nonzero(pv.var_converged))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=["large", "accuracy"], default=None)
    args = ap.parse_args()
    if args.step == "large":
        return step_large(args)
    if args.step == "accuracy":
        return step_accuracy(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--m", str(args.m), "--reps", str(args.reps)]
    steps = [("large", ["--N", str(args.N)])]
    if args.N != 16000:
        steps.append(("large", ["--N", "16000"]))
    steps.append(("accuracy", []))
    for name, extra in steps:
        rc = subprocess.run(base + ["--step", name] + extra).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
