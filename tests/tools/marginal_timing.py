"""Times of the prediction averaged over hyperparameter samples on one MI355X, median of --reps (after one warm-up), as JSON lines:

 batch   64 emulators x n = 2000 x D = 10, S = 32 samples each, m = 10^4 query points: one ``predict_marginal`` call against the hand
         loop over the same samples -- ``fit(theta_s)`` + ``predict`` + a NumPy reduction, then the MAP fit put back --, which needs
         nothing of the mixture call and runs on older builds too;
 single  one n = 2000 emulator, the same.

Both with the largest difference of the two results (they add the samples up in different orders) and the device time of the
reduction kernel (tag mixture_accumulate).

    python tests/tools/marginal_timing.py [--n 2000] [--D 10] [--batch 64] [--samples 32] [--m 10000] [--reps 5] [--limit 600]

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


def median_time(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, out


def kernel_ms(lib, fn, tag):
    lib.mogp_profile_reset()
    lib.mogp_profile_enable(1)
    fn()
    lib.mogp_profile_enable(0)
    ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
    if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0:
        return {"ms": ms.value, "launches": cnt.value}
    return None


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D, S, m = args.n, args.D, args.samples, args.m
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    Xs = rng.random((m, D))
    hat = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    thetas = hat + 0.05 * rng.standard_normal((B, S, hat.size))
    w = np.full(S, 1. / S)
    have = hasattr(M, "predict_marginal")
    if args.step == "batch":
        gp = M.MultiOutputGP_GPU(X, T, nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
        gp.fit(np.tile(hat, (B, 1)))
        call = lambda: M.predict_marginal(gp, Xs, thetas=thetas)                   # noqa: E731

        def loop():
            mus, vs = np.zeros((S, B, m)), np.zeros((S, B, m))
            for s in range(S):
                gp.fit(thetas[:, s])
                p = gp.predict(Xs, deriv=False)
                mus[s], vs[s] = p.mean, p.unc
            gp.fit(np.tile(hat, (B, 1)))                                           # the MAP fit back in place
            mean = np.tensordot(w, mus, 1)
            return mean, np.tensordot(w, vs, 1), np.tensordot(w, (mus - mean) ** 2, 1)
    else:
        gp = M.GaussianProcessGPU(X, T[0], nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"), max_batch_size=m)
        gp.fit(hat)
        call = lambda: M.predict_marginal(gp, Xs, thetas=thetas[0])                # noqa: E731

        def loop():
            mus, vs = np.zeros((S, m)), np.zeros((S, m))
            for s in range(S):
                gp.fit(thetas[0, s])
                p = gp.predict(Xs, deriv=False)
                mus[s], vs[s] = p.mean, p.unc
            gp.fit(hat)
            mean = w @ mus
            return mean, w @ vs, w @ (mus - mean) ** 2
    t_l, all_l, ref = median_time(loop, max(1, args.reps // 2))
    out = {"step": args.step, "n": n, "D": D, "emulators": B, "samples": S, "m": m, "hand_loop_s": t_l, "hand_loop_all_s": all_l}
    if have:
        t_c, all_c, res = median_time(call, args.reps)
        out.update(predict_marginal_s=t_c, predict_marginal_all_s=all_c, ratio=t_l / t_c,
                   max_abs_diff={"mean": float(np.abs(res.mean - ref[0]).max()), "within": float(np.abs(res.within - ref[1]).max()),
                                 "between": float(np.abs(res.between - ref[2]).max())},
                   accumulate_kernel=kernel_ms(lib, call, "mixture_accumulate"))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("single", "batch"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--samples", str(args.samples), "--m", str(args.m), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
