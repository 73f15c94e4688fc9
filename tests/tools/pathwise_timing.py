"""Times of the pathwise posterior draws (mogp_emulator_amd.IterativeGP.sample_paths, PosteriorPaths.evaluate) on one MI355X, as JSON lines.
Squared exponential, D = 10, hyperparameters of an emulator fitted at a fixed theta on a 2000-point subsample (those of
tests/tools/iterative_timing.py), preconditioner rank 1024, rtol 1e-8:

 paths     N design points (default 16 000 and 10^5), F = 2048 / 4096 features, S = 16 / 32 draws, m = 10^4 queries:
             sample_s     wall time of sample_paths (the preconditioner already built): the weights' normals, g_s(X), the right-hand sides
                          and the solve, all on the device
             evaluate_s   wall time of evaluate at the m queries;  rff_ms: the feature kernel's HIP-event time at the design
             baseline     the same computation composed from what the class had before: a host NumPy feature matrix cos(X~ omega^T + b)
                          (N x F doubles) times W, ``solve`` of the right-hand sides, and at the queries the host feature matrix plus
                          ``matvec(testing=)`` -- sample_s, evaluate_s and the largest difference of the two evaluations
 accuracy  N = 16 000, 64 queries, 256 draws: the gap of the sample mean and of the sample variance of the paths (F = 4096) to those of
           the dense ``sample_posterior`` with as many draws, and to the dense ``predict``, relative to the spread of the targets / the
           mean predictive variance.

    python tests/tools/pathwise_timing.py [--N 16000,100000] [--F 2048,4096] [--S 16,32] [--m 10000] [--limit 900]

Every step is a child process under its own ``timeout``; a step that fails, or runs out of time, ends the run (nothing further is started
on the device).  Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from iterative_timing import RTOL, MAX_ITER, data, fitted, kernel_ms, note, wall      # noqa: E402

RANK = 1024


def step_paths(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Sampling import philox_normals
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, m, F, S = args.n, args.D, args.m, args.f, args.s
    X, t, Q = data(N, D, m)
    gp, theta = fitted(X, t, D, 2000)
    ig = M.IterativeGP(gp, X, t, precond_rank=RANK, rtol=RTOL, max_iter=MAX_ITER)
    kt, s, sigma2, eta = ig._hyper[0][:4]
    build_s = wall(lambda: ig._native.precondition(kt, s, sigma2, eta, RANK))[0]
    out = {"step": "paths", "N": N, "D": D, "m": m, "F": F, "S": S, "rank": RANK, "rtol": RTOL, "precondition_s": build_s}
    ig.sample_paths(1, n_features=64, seed=1)                            # warm-up: the kernels are loaded
    sample_s, paths = wall(lambda: ig.sample_paths(S, n_features=F, seed=1))
    evaluate_s, f = wall(lambda: paths.evaluate(Q))
    out.update(sample_s=sample_s, evaluate_s=evaluate_s, iterations=paths.iterations.tolist(), converged=int(np.count_nonzero(paths.converged)),
               largest_residual=float(paths.residual.max()))
    W, amp = paths.feature_normals, np.sqrt(2. * sigma2 / F)
    out["rff_ms"] = kernel_ms(lib, lambda: ig._native.rff(s, paths.omega, paths.phase, W, amp), "rff", args.reps)
    note("device", out)
    eps = philox_normals(1, paths.stream + 4, S, N)

    def base_sample():
        Phi = np.cos((X * s) @ paths.omega.T + paths.phase[None, :])
        b = t[:, None] - amp * (Phi @ W.T) - np.sqrt(eta) * eps.T
        return ig.solve(np.ascontiguousarray(b))

    def base_evaluate(v):
        Phi = np.cos((Q * s) @ paths.omega.T + paths.phase[None, :])
        return (amp * (Phi @ W.T) + ig.matvec(v, testing=Q)).T
    bs, sv = wall(base_sample)
    be, fb = wall(lambda: base_evaluate(sv.x))
    out["baseline"] = {"sample_s": bs, "evaluate_s": be, "iterations": sv.iterations.tolist(), "largest_difference": float(np.max(np.abs(fb - f)))}
    ig.close()
    print(json.dumps(out))


def step_accuracy(args):
    import mogp_emulator_amd as M
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D, m, S, F = 16000, args.D, 64, 256, 4096
    X, t, Q = data(N, D, m, seed=2)
    gp, theta = fitted(X, t, D, N)
    dense = gp.predict(Q, deriv=False)
    sd, vbar = float(np.std(t)), float(np.mean(dense.unc - gp.nugget))
    ref = M.sample_posterior(gp, Q, n_draws=S, rng=3, include_nugget=False)
    ig = M.IterativeGP(gp, X, t, precond_rank=RANK, rtol=RTOL, max_iter=MAX_ITER)
    s, paths = wall(lambda: ig.sample_paths(S, n_features=F, seed=3))
    f = paths.evaluate(Q)
    ig.close()
    mean_p, var_p = f.mean(axis=0), f.var(axis=0, ddof=1)
    mean_d, var_d = ref.samples.mean(axis=0), ref.samples.var(axis=0, ddof=1)
    print(json.dumps({"step": "accuracy", "N": N, "D": D, "m": m, "S": S, "F": F, "sample_s": s, "converged": int(np.count_nonzero(paths.converged)),
                      "target_std": sd, "mean_predictive_variance": vbar,
                      "sample_mean_gap_to_dense_samples_over_target_std": float(np.max(np.abs(mean_p - mean_d)) / sd),
                      "sample_mean_gap_to_predict_over_target_std": float(np.max(np.abs(mean_p - dense.mean)) / sd),
                      "dense_samples_mean_gap_to_predict_over_target_std": float(np.max(np.abs(mean_d - dense.mean)) / sd),
                      "mean_sample_variance_over_predictive": float(np.mean(var_p) / vbar),
                      "dense_samples_mean_sample_variance_over_predictive": float(np.mean(var_d) / vbar)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="16000,100000")
    ap.add_argument("--F", default="2048,4096")
    ap.add_argument("--S", default="16,32")
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=["paths", "accuracy"], default=None)
    ap.add_argument("--n", type=int, default=16000)
    ap.add_argument("--f", type=int, default=2048)
    ap.add_argument("--s", type=int, default=16)
    ap.add_argument("--no-accuracy", action="store_true")
    args = ap.parse_args()
    if args.step == "paths":
        return step_paths(args)
    if args.step == "accuracy":
        return step_accuracy(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--m", str(args.m), "--reps", str(args.reps)]
    steps = [("paths", ["--n", n, "--f", f, "--s", s]) for n in args.N.split(",") for f in args.F.split(",") for s in args.S.split(",")]
    if not args.no_accuracy:
        steps.append(("accuracy", []))
    for name, extra in steps:
        rc = subprocess.run(base + ["--step", name] + extra).returncode
        if rc != 0:
            raise SystemExit("step %s %s ended with status %d: nothing further is started" % (name, " ".join(extra), rc))


if __name__ == "__main__":
    main()
