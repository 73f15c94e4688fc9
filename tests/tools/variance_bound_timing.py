"""Times and accuracy of the variance bound (mogp_emulator_amd.IterativeGP.variance_bound) on one MI355X, as JSON lines.  Squared
exponential, D = 10, hyperparameters of an emulator fitted at a fixed theta on a 2000-point subsample: the setting of iterative_timing.py,
whose data and emulator this tool takes.

 large     per N (default 16 000 and 10^5) and per preconditioner rank p (256 and 1024):
             precondition   wall time of the preconditioner's build (the bound's cache starts from its factor)
             cache          wall time of the first variance_cache-building call on top of it, and the rank of the cache
             bound          m = 10^4 bounds: wall time of the call (min / median / max of --reps) and the HIP-event time of its kernels
             composition    the same numbers without the fused kernel: matvec(R[:, 32 b : 32 b + 32], testing=) for every block b and the
                            squares summed in NumPy (min / median / max of --reps, at most --comp-blocks blocks timed and scaled to all of
                            them; the cache's download is not counted)
             exact          predict(unc=True) on 256 queries at p = 256: the unchanged exact path, one solve per query (--no-exact skips it)
 accuracy  N = 16 000, 2000 queries, p = 256 and 1024: mean and maximum of (bound - dense) / sigma^2 and of bound / dense against the dense
           ``GaussianProcessGPU.predict`` at the same hyperparameters, and the smallest difference.

    python tests/tools/variance_bound_timing.py [--N 16000 100000] [--ranks 256 1024] [--m 10000] [--reps 3] [--limit 900]

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

from iterative_timing import MAX_ITER, RTOL, data, fitted, kernel_ms, note, wall      # noqa: E402


def spread(times):
    return {"min_s": min(times), "median_s": statistics.median(times), "max_s": max(times), "reps": len(times)}


def step_large(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D, m, p = args.N[0], args.D, args.m, args.ranks[0]
    X, t, Q = data(N, D, m)
    gp, theta = fitted(X, t, D, 2000)
    out = {"step": "large", "N": N, "D": D, "m": m, "p": p, "nugget": float(gp.nugget)}
    ig = M.IterativeGP(gp, X, t, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
    s, (rank, _) = wall(lambda: ig._native.precondition(*ig._hyper[0][:4], p)[:2])
    out["precondition"] = {"build_s": s, "rank": int(rank)}
    s, first = wall(lambda: ig.variance_bound(Q[:64]))
    out["cache"] = {"build_and_64_bounds_s": s}
    note("cache", out["cache"])
    times = [wall(lambda: ig.variance_bound(Q))[0] for _ in range(args.reps)]
    out["bound"] = dict(spread(times), kernel_ms=kernel_ms(lib, lambda: ig.variance_bound(Q), "kvar", args.reps))
    note("bound", out["bound"])
    got = ig.variance_bound(Q)
    R, vrank = ig.variance_cache()
    out["cache"]["var_rank"] = int(vrank)
    sigma2, nugget = ig._hyper[0][2], ig._hyper[0][3]
    blocks = [(b, min(b + 32, vrank)) for b in range(0, vrank, 32)]
    timed = blocks[:args.comp_blocks]

    def composition(which):
        q = np.zeros(m)
        for lo, hi in which:
            w = ig.matvec(np.ascontiguousarray(R[:, lo:hi]), testing=Q)
            q += np.sum(w * w, axis=1)
        return np.maximum(sigma2 + nugget - q, 0.)
    scale = len(blocks) / float(len(timed))
    times = [wall(lambda: composition(timed))[0] * scale for _ in range(args.reps)]
    out["composition"] = dict(spread(times), blocks=len(blocks), blocks_timed=len(timed),
                              kernel_ms_per_block=kernel_ms(lib, lambda: composition(timed[:1]), "kmatvec", args.reps))
    if len(timed) == len(blocks):
        out["composition"]["largest_difference_over_sigma2"] = float(np.max(np.abs(composition(blocks) - got)) / sigma2)
    note("composition", out["composition"])
    if not args.no_exact and p == 256:
        s, pv = wall(lambda: ig.predict(Q[:256], unc=True))
        out["exact"] = {"m": 256, "predict_s": s, "converged": int(np.count_nonzero(pv.var_converged))}
        gap = got[:256] - pv.unc
        out["exact"]["bound_minus_exact_over_sigma2"] = {"mean": float(gap.mean() / sigma2), "max": float(gap.max() / sigma2),
                                                         "min": float(gap.min() / sigma2)}
    ig.close()
    print(json.dumps(out), flush=True)


def step_accuracy(args):
    import mogp_emulator_amd as M
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D, m = 16000, args.D, 2000
    X, t, Q = data(N, D, m, seed=2)
    gp, theta = fitted(X, t, D, N)
    dense = gp.predict(Q, deriv=False).unc
    out = {"step": "accuracy", "N": N, "D": D, "m": m}
    for p in args.ranks:
        ig = M.IterativeGP(gp, X, t, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        b = ig.variance_bound(Q)
        sigma2, vrank = ig._hyper[0][2], ig.variance_cache()[1]
        ig.close()
        out["p%d" % p] = {"var_rank": int(vrank), "gap_over_sigma2_mean": float(np.mean(b - dense) / sigma2),
                          "gap_over_sigma2_max": float(np.max(b - dense) / sigma2), "gap_over_sigma2_min": float(np.min(b - dense) / sigma2),
                          "ratio_mean": float(np.mean(b / dense)), "ratio_max": float(np.max(b / dense)),
                          "dense_over_sigma2_mean": float(np.mean(dense) / sigma2)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[16000, 100000])
    ap.add_argument("--ranks", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--comp-blocks", type=int, default=32, help="blocks of 32 columns of the composition that are timed (the rest is scaled)")
    ap.add_argument("--no-exact", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--limit", type=int, default=900, help="seconds per step")
    ap.add_argument("--step", choices=["large", "accuracy"], default=None)
    args = ap.parse_args()
    if args.step == "large":
        return step_large(args)
    if args.step == "accuracy":
        return step_accuracy(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D), "--m", str(args.m), "--reps",
            str(args.reps), "--comp-blocks", str(args.comp_blocks)] + (["--no-exact"] if args.no_exact else [])
    steps = [("large", ["--N", str(N), "--ranks", str(p)]) for N in args.N for p in args.ranks if p <= N]
    if not args.no_accuracy:
        steps.append(("accuracy", ["--ranks"] + [str(p) for p in args.ranks]))
    for name, extra in steps:
        rc = subprocess.run(base + ["--step", name] + extra).returncode
        if rc != 0:
            raise SystemExit("step %s %s ended with status %d: nothing further is started" % (name, " ".join(extra), rc))


if __name__ == "__main__":
    main()
