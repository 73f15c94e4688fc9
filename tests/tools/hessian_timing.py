"""Times of the log-posterior Hessian on one MI355X, median of --reps (after one warm-up), as JSON lines:

 batch   64 emulators x n = 2000 x D = 10, one ``MultiOutputGP_GPU.hessian`` call, against 2 P batched fit + gradient evaluations
         (``eval``) -- what a central difference of the gradient costs (P = D + 1 + [nugget fitted]);
 single  one n = 2000 emulator, ``logpost_hessian`` against 2 P ``fit`` + ``logpost_deriv``.

Both on the same build, with the device time of the kernels by tag (hess_planes, hess_trace, hess_pair, hess_vectors).

    python tests/tools/hessian_timing.py [--n 2000] [--D 10] [--batch 64] [--reps 5] [--limit 600]

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
TAGS = ("hess_planes", "hess_trace", "hess_pair", "hess_vectors", "grad_reduce", "kinv")


def median_time(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def kernel_ms(lib, fn):
    lib.mogp_profile_reset()
    lib.mogp_profile_enable(1)
    fn()
    lib.mogp_profile_enable(0)
    out = {}
    for tag in TAGS:
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0:
            out[tag] = {"ms": ms.value, "launches": cnt.value, "flops": fl.value}
    return out


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D = args.n, args.D
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    theta = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    P = theta.size
    h = 1e-5
    if args.step == "batch":
        mo = M.MultiOutputGP_GPU(X, T, nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
        rows = np.tile(theta, (B, 1)) + 0.01 * rng.standard_normal((B, P))
        call = lambda: mo._mogp_gpu.hessian(rows)                                  # noqa: E731

        def fd():
            for j in range(P):
                for sgn in (1., -1.):
                    r = rows.copy()
                    r[:, j] += sgn * h
                    mo._mogp_gpu.eval(r, grad=True)
    else:
        gp = M.GaussianProcessGPU(X, T[0], nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
        call = lambda: M.logpost_hessian(gp, theta)                                # noqa: E731

        def fd():
            for j in range(P):
                for sgn in (1., -1.):
                    r = theta.copy()
                    r[j] += sgn * h
                    gp.logpost_deriv(r)
    t_h, all_h = median_time(call, args.reps)
    t_fd, all_fd = median_time(fd, max(1, args.reps // 2))
    print(json.dumps({"step": args.step, "n": n, "D": D, "emulators": B, "P": P, "hessian_s": t_h, "hessian_all_s": all_h,
                      "finite_difference_s": t_fd, "finite_difference_all_s": all_fd, "evaluations": 2 * P, "ratio": t_fd / t_h,
                      "algorithmic_tflops_planes": 2. * D * n ** 3 * B / 1e12, "kernels": kernel_ms(lib, call)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("batch", "single"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
