"""Times of the ALC criterion on one MI355X, median of --reps (after one warm-up), as JSON lines:

 single  one n = 2000 x D = 10 emulator, m_c = 5000 candidates against m_r = 10^4 reference points: one ``alc_criterion`` call against
         the only route without it on the same build --
           host      ``predict(full_cov=True)`` on the stacked points [candidates; reference] (an (m_c + m_r)^2 matrix per emulator to the
                     host), in as many calls as its 64 GB rule forces, then the reduction in NumPy;
 batch   16 emulators, the same (the baseline once, after no warm-up: it moves 29 GB; left out where the host has no room for it).

Beside it the HIP-event time of the kernel (tag alc_cross, 2 n m_c m_r flops per emulator) with its rate, the rate ``fullcov_syrk`` reaches
on the same machine at the same n (one ``predict(full_cov=True)`` at m_c points), and the largest relative difference of the two results.

    python tests/tools/alc_timing.py [--n 2000] [--D 10] [--batch 16] [--mc 5000] [--mr 10000] [--reps 5] [--limit 600]

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


def host_mem_available():
    try:
        with open("/proc/meminfo") as f:
            for ln in f:
                if ln.startswith("MemAvailable:"):
                    return int(ln.split()[1]) * 1024
    except OSError:
        pass
    return None


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D, mc, mr = args.n, args.D, args.mc, args.mr
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    cand, ref = rng.random((mc, D)), rng.random((mr, D))
    hat = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    pri = GPPriors(n_corr=D, nugget_type="fit")
    if args.step == "batch":
        gp = M.MultiOutputGP_GPU(X, T, nugget="fit", priors=pri)
        gp.fit(np.tile(hat, (B, 1)))
        nuggets = np.asarray(gp._nuggets())
    else:
        gp = M.GaussianProcessGPU(X, T[0], nugget="fit", priors=pri)
        gp.fit(hat)
        nuggets = np.array([gp.nugget])
    w = np.full(mr, 1. / mr)
    stacked = np.vstack([cand, ref])

    def host():
        cov = np.reshape(gp.predict(stacked, full_cov=True, include_nugget=False, deriv=False).unc, (B, mc + mr, mc + mr))
        out = np.zeros((B, mc))
        for e in range(B):
            d = np.maximum(np.diag(cov[e])[:mc], 0.) + nuggets[e]
            out[e] = (cov[e][:mc, mc:] ** 2 @ w) / d
        return out

    call = lambda: M.alc_criterion(gp, cand, ref)                         # noqa: E731
    t_c, all_c, res = median_time(call, args.reps)
    out = {"step": args.step, "n": n, "D": D, "emulators": B, "m_c": mc, "m_r": mr, "alc_criterion_s": t_c, "alc_criterion_all_s": all_c,
           "degenerate": int(res.degenerate.sum()), "kernels": kernel_ms(lib, call, ("alc_cross", "cross_cov", "predict_var"))}
    out["kernels_fullcov_at_m_c"] = kernel_ms(lib, lambda: gp.predict(cand, full_cov=True, include_nugget=False, deriv=False),
                                              ("fullcov_syrk", "predict_var"))
    need = 8. * B * (mc + mr) ** 2 * 2.2
    avail = host_mem_available()
    if avail is not None and avail < need:
        out["host_skipped"] = "the baseline needs %.0f GB of host memory, %.0f GB are available" % (need / 1e9, avail / 1e9)
    else:
        t_h, all_h, base = median_time(host, 1 if B > 1 else max(1, args.reps // 2), warm=(B == 1))
        out.update({"host_s": t_h, "host_all_s": all_h, "host_ratio": t_h / t_c,
                    "max_rel_diff_host": float(np.max(np.abs(res.reduction - base) / base))})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--mc", type=int, default=5000)
    ap.add_argument("--mr", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("single", "batch"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--mc", str(args.mc), "--mr", str(args.mr), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
