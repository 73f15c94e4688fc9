"""Times of joint posterior draws on one MI355X, median of --reps (after one warm-up), as JSON lines:

 single  one n = 2000 x D = 10 emulator, m = 2000 query points, S = 1000 draws: one ``sample_posterior`` call against what a user does
         without it on the same build --
           host      ``predict(full_cov=True)`` (m x m doubles per emulator to the host), ``np.linalg.cholesky`` per emulator with the same
                     jitter ladder, ``rng.standard_normal`` and one matrix product per emulator;
 batch   64 emulators, the same.

With the device times of the four kernels (tags sample_gather, sample_polish, sample_normals, sample_apply) and, for the same normals, the largest
difference of the two results.

    python tests/tools/sample_timing.py [--n 2000] [--D 10] [--batch 64] [--m 2000] [--draws 1000] [--reps 5] [--limit 600]

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


def host_factor(cov, nugget):
    """chol(cov + nugget I) with the ladder of the device call: (L, jitter used)"""
    m = cov.shape[0]
    dbar = float(np.mean(np.diag(cov)))
    for delta in [0.] + [dbar * 1e-6 * 10. ** t for t in range(5)]:
        try:
            return np.linalg.cholesky(cov + (nugget + delta) * np.eye(m)), delta
        except np.linalg.LinAlgError:
            pass
    return None, np.nan


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D, m, S = args.n, args.D, args.m, args.draws
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    Xs = rng.random((m, D))
    hat = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    pri = GPPriors(n_corr=D, nugget_type="fit")
    if args.step == "batch":
        gp = M.MultiOutputGP_GPU(X, T, nugget="fit", priors=pri)
        gp.fit(np.tile(hat, (B, 1)))
        nuggets = gp._nuggets()
    else:
        gp = M.GaussianProcessGPU(X, T[0], nugget="fit", priors=pri)
        gp.fit(hat)
        nuggets = np.array([gp.nugget])

    def host(z=None):
        p = gp.predict(Xs, full_cov=True, include_nugget=False, deriv=False)
        mean, cov = np.reshape(p.mean, (B, m)), np.reshape(p.unc, (B, m, m))
        g = np.random.default_rng(2)
        out = np.zeros((B, S, m))
        for e in range(B):
            L, _ = host_factor(cov[e], nuggets[e])
            ze = g.standard_normal((S, m)) if z is None else z[e]
            out[e] = mean[e] + ze @ L.T
        return out

    call = lambda: M.sample_posterior(gp, Xs, n_draws=S, rng=3)                         # noqa: E731
    t_c, all_c, res = median_time(call, args.reps)
    t_h, all_h, _ = median_time(host, max(1, args.reps // 2))
    with_z = M.sample_posterior(gp, Xs, n_draws=S, rng=3, return_z=True)
    ref = host(np.reshape(with_z.z, (B, S, m)))
    out = {"step": args.step, "n": n, "D": D, "emulators": B, "m": m, "draws": S, "sample_posterior_s": t_c, "sample_posterior_all_s": all_c,
           "host_s": t_h, "host_all_s": all_h, "host_ratio": t_h / t_c, "ok": bool(np.all(res.ok)),
           "jitter_used_max": float(np.max(res.jitter_used)), "max_abs_diff_host": float(np.abs(np.reshape(with_z.samples, (B, S, m)) - ref).max()),
           "kernels": kernel_ms(lib, call, ("sample_gather", "sample_polish", "sample_normals", "sample_apply"))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--m", type=int, default=2000)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("single", "batch"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--m", str(args.m), "--draws", str(args.draws), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
