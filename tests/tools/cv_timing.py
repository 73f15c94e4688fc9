"""Times of cross-validation at the fitted hyperparameters on one MI355X, median of --reps (after one warm-up), as JSON lines:

 batch   64 emulators x n = 2000 x D = 10, k = 10 folds and leave-one-out: one ``cross_validate`` call against the two things a user does
         without it on the same build --
           refits    k models of the other folds at the fitted theta (``MultiOutputGP_GPU`` / ``GaussianProcessGPU``: construct, ``fit``,
                     ``predict`` the held-out fold); k = 10 only -- n refits of n - 1 points are not something anybody waits for;
           host      ``get_invQ`` of every emulator (n x n doubles each) to the host and the block solves in NumPy;
 single  one n = 2000 emulator, the same.

With the largest difference of the results and the device times of the three kernels (tags cv_gather, cv_finish, cv_loo).

    python tests/tools/cv_timing.py [--n 2000] [--D 10] [--batch 64] [--k 10] [--reps 5] [--limit 600]

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


def kernel_ms(lib, fn, tags):
    lib.mogp_profile_reset()
    lib.mogp_profile_enable(1)
    fn()
    lib.mogp_profile_enable(0)
    out = {}
    for tag in tags:
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0:
            out[tag] = {"ms": ms.value, "launches": cnt.value}
    return out


def host_blocks(Qinv, alpha, t, labels, k):
    """the fast form in NumPy from the full inverse: (mean, var) of one emulator"""
    mean, var = np.zeros_like(t), np.zeros_like(t)
    for f in range(k):
        F = np.flatnonzero(labels == f)
        Sigma = np.linalg.inv(Qinv[np.ix_(F, F)])
        mean[F] = t[F] - Sigma @ alpha[F]
        var[F] = np.diag(Sigma)
    return mean, var


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D, k = args.n, args.D, args.k
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    hat = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    pri = GPPriors(n_corr=D, nugget_type="fit")
    labels = M.kfold_labels(n, k)
    if args.step == "batch":
        gp = M.MultiOutputGP_GPU(X, T, nugget="fit", priors=pri)
        gp.fit(np.tile(hat, (B, 1)))
        natives = [gp._mogp_gpu.emulator(e) for e in range(B)]

        def refits():
            mean, var = np.zeros((B, n)), np.zeros((B, n))
            for f in range(k):
                F = labels == f
                part = M.MultiOutputGP_GPU(X[~F], T[:, ~F], nugget="fit", priors=pri)
                part.fit(np.tile(hat, (B, 1)))
                p = part.predict(X[F], deriv=False)
                mean[:, F], var[:, F] = p.mean, p.unc
            return mean, var
    else:
        gp = M.GaussianProcessGPU(X, T[0], nugget="fit", priors=pri)
        gp.fit(hat)
        natives = [gp._densegp_gpu]

        def refits():
            mean, var = np.zeros((1, n)), np.zeros((1, n))
            for f in range(k):
                F = labels == f
                part = M.GaussianProcessGPU(X[~F], T[0, ~F], nugget="fit", priors=pri)
                part.fit(hat)
                p = part.predict(X[F], deriv=False)
                mean[0, F], var[0, F] = p.mean, p.unc
            return mean, var

    def host(lab, kk):
        mean, var = np.zeros((B, n)), np.zeros((B, n))
        Qinv, alpha = np.zeros((n, n)), np.zeros(n)
        for e, nat in enumerate(natives):
            nat.get_invQ(Qinv)
            nat.get_invQt(alpha)
            if kk == n:
                d = np.diag(Qinv)
                mean[e], var[e] = T[e] - alpha / d, 1. / d
            else:
                mean[e], var[e] = host_blocks(Qinv, alpha, T[e], lab, kk)
        return mean, var

    out = {"step": args.step, "n": n, "D": D, "emulators": B, "k": k}
    for name, kw, lab, kk in (("kfold", dict(k=k), labels, k), ("loo", dict(), np.arange(n), n)):
        call = lambda: M.cross_validate(gp, **kw)                                  # noqa: E731
        t_c, all_c, res = median_time(call, args.reps)
        t_h, all_h, ref_h = median_time(lambda: host(lab, kk), max(1, args.reps // 2))
        row = {"cross_validate_s": t_c, "cross_validate_all_s": all_c, "host_invQ_s": t_h, "host_invQ_all_s": all_h, "host_ratio": t_h / t_c,
               "max_abs_diff_host": {"mean": float(np.abs(np.reshape(res.mean, (B, n)) - ref_h[0]).max()),
                                     "var": float(np.abs(np.reshape(res.unc, (B, n)) - ref_h[1]).max())},
               "kernels": kernel_ms(lib, call, ("cv_gather", "cv_finish", "cv_loo"))}
        if name == "kfold":
            t_r, all_r, ref_r = median_time(refits, max(1, args.reps // 2))
            row.update(refits_s=t_r, refits_all_s=all_r, refits_ratio=t_r / t_c,
                       max_abs_diff_refits={"mean": float(np.abs(np.reshape(res.mean, (B, n)) - ref_r[0]).max()),
                                            "var": float(np.abs(np.reshape(res.unc, (B, n)) - ref_r[1]).max())})
        out[name] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("single", "batch"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--k", str(args.k), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
