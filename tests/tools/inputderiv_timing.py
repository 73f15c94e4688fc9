"""Times of the input derivatives at large designs (mogp_emulator_amd.PosteriorPaths.gradient and its two kernels) on one MI355X, as JSON
lines.  The setting of tests/tools/pathwise_timing.py: squared exponential, D = 10, hyperparameters of an emulator fitted at a fixed theta on a
2000-point subsample, preconditioner rank 1024, rtol 1e-8, S = 32 paths of F = 2048 features, m = 10^4 queries, N = 16 000 and 10^5.

 gradient_s      wall time of PosteriorPaths.gradient at the m queries (median of the repeats after a warm-up); kinderiv_ms / rff_inderiv_ms:
                 the two kernels' HIP-event times of one call, kmatvec_ms that of the product one ``evaluate`` runs
 central_s       what a user had before: 2 D calls of ``evaluate`` on query sets moved by +- h e_d, h = 1e-5 / s_d, and their difference;
                 central_gap: its largest distance from ``gradient`` relative to the largest entry
 expanded_s      for the squared exponential k' = -k / 2: the expanded composition q~_d (K v) - K (x~_d * v) through ``matvec(testing=)`` on
                 the panels [v | x~_d * v] ((D + 1) S columns) plus ``prior_gradient``
 fractions       on the first `--check` queries, of the bar of tests/inputderiv_restate.py against its long-double form: the device's sweep
                 and the expanded composition

    python tests/tools/inputderiv_timing.py [--N 16000,100000] [--F 2048] [--S 32] [--m 10000] [--reps 3] [--check 8] [--limit 900]

Every step is a child process under its own ``timeout``; a step that fails, or runs out of time, ends the run (nothing further is started
on the device).  Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from iterative_timing import RTOL, MAX_ITER, data, fitted, kernel_ms, note, wall      # noqa: E402

RANK = 1024


def median_wall(fn, reps):
    fn()                                                      # warm-up
    times, out = [], None
    for _ in range(reps):
        t, out = wall(fn)
        times.append(t)
    return statistics.median(times), out


def step_gradient(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    import inputderiv_restate as idr
    import iterative_restate as ir
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, m, F, S = args.n, args.D, args.m, args.f, args.s
    X, t, Q = data(N, D, m)
    gp, theta = fitted(X, t, D, 2000)
    ig = M.IterativeGP(gp, X, t, precond_rank=RANK, rtol=RTOL, max_iter=MAX_ITER)
    kt, s, sigma2, eta = ig._hyper[0][:4]
    paths = ig.sample_paths(S, n_features=F, seed=1)
    v, W, amp = paths.update, paths.feature_normals, np.sqrt(2. * sigma2 / F)
    out = {"step": "gradient", "N": N, "D": D, "m": m, "F": F, "S": S, "rank": RANK, "converged": int(np.count_nonzero(paths.converged))}
    out["gradient_s"], g = median_wall(lambda: paths.gradient(Q), args.reps)
    out["evaluate_s"] = median_wall(lambda: paths.evaluate(Q), args.reps)[0]
    out["kinderiv_ms"] = kernel_ms(lib, lambda: ig._native.kmatvec_inputderiv(kt, s, sigma2, v, Q), "kinderiv", args.reps)
    out["rff_inderiv_ms"] = kernel_ms(lib, lambda: ig._native.rff_inputderiv(s, paths.omega, paths.phase, W, amp, Q), "rff_inderiv", args.reps)
    out["kmatvec_ms"] = kernel_ms(lib, lambda: ig._native.kmatvec(kt, s, sigma2, eta, v, queries=Q), "kmatvec", args.reps)
    note("device", out)

    def central():
        fd = np.empty((S, m, D))
        for d in range(D):
            h = 1e-5 / s[d]
            Qp, Qm = Q.copy(), Q.copy()
            Qp[:, d] += h
            Qm[:, d] -= h
            fd[:, :, d] = (paths.evaluate(Qp) - paths.evaluate(Qm)) / (Qp[:, d] - Qm[:, d])[None, :]
        return fd
    out["central_s"], fd = median_wall(central, args.reps)
    out["central_gap"] = float(np.max(np.abs(fd - g)) / np.max(np.abs(g)))
    if kt == 0:
        Xt = ir.scaled(X, s)
        panel = np.ascontiguousarray(np.hstack([v] + [Xt[:, d][:, None] * v for d in range(D)]))       # (N, (D + 1) S)

        def expanded(queries):
            P = ig.matvec(panel, testing=queries)
            Qt = ir.scaled(queries, s)
            G = np.stack([-s[d] * (Qt[:, d][:, None] * P[:, :S] - P[:, (d + 1) * S:(d + 2) * S]) for d in range(D)], axis=1)      # (m, D, S)
            return paths.prior_gradient(queries) + np.transpose(G, (2, 0, 1)), G
        out["expanded_s"], (ge, _) = median_wall(lambda: expanded(Q), args.reps)
        out["expanded_gap"] = float(np.max(np.abs(ge - g)) / np.max(np.abs(g)))
    nq = args.check
    if nq > 0 and np.finfo(np.longdouble).eps < 2. ** -60:
        Qc = Q[:nq]
        Qt, Xt = ir.scaled(Qc, s), ir.scaled(X, s)
        kind = "SquaredExponential" if kt == 0 else "Matern52"
        truth = idr.kgrad_in(Qt, Xt, s, kind, sigma2, v, dtype=np.longdouble)
        bar = idr.kgrad_bar(Qt, Xt, s, kind, sigma2, v)

        def frac(got):
            return float(np.max(np.abs(np.asarray(got.astype(np.longdouble) - truth, dtype=np.float64)) / bar))
        out["sweep_fraction_of_bar"] = frac(ig._native.kmatvec_inputderiv(kt, s, sigma2, v, Qc))
        if kt == 0:
            out["expanded_fraction_of_bar"] = frac(expanded(Qc)[1])
    ig.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="16000,100000")
    ap.add_argument("--F", default="2048")
    ap.add_argument("--S", default="32")
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=8, help="queries of the accuracy check (0: none)")
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=["gradient"], default=None)
    ap.add_argument("--n", type=int, default=16000)
    ap.add_argument("--f", type=int, default=2048)
    ap.add_argument("--s", type=int, default=32)
    args = ap.parse_args()
    if args.step == "gradient":
        return step_gradient(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--m", str(args.m), "--reps", str(args.reps),
            "--check", str(args.check)]
    for n in args.N.split(","):
        for f in args.F.split(","):
            for s in args.S.split(","):
                rc = subprocess.run(base + ["--step", "gradient", "--n", n, "--f", f, "--s", s]).returncode
                if rc != 0:
                    raise SystemExit("step gradient %s %s %s ended with status %d: nothing further is started" % (n, f, s, rc))


if __name__ == "__main__":
    main()
