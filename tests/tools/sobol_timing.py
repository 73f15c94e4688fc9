"""Time of the fused sensitivity analysis on one MI355X against the path a user had before it, in one process:

 1. ``sobol_indices(mo, A=A, B=B)`` -- A and B uploaded once, every AB_i built on the device, 2 D + 3 numbers per emulator returned;
 2. the same (D + 2) N points through ``MultiOutputGP_GPU.predict(unc=False, deriv=False)`` (points uploaded, means downloaded) and the
    NumPy restatement of the estimators (tests/sobol_restate.py);
 3. the device time of the fused call's kernels by tag (HIP events of the library's profiling registry, taken in a run of their own):
    pick-freeze, the mean path (cross covariance), the reductions.

Default configuration: 64 emulators x n = 2000 x D = 10, N = 65 536.  One warm-up each, then ``--reps`` repeats taken alternately (so
that a drift of the clocks hits both paths alike); medians and the min-max spread are reported, one JSON line at the end.  Exit status 1
when the fused call is slower than the existing path by more than the 2 % box-to-box spread.

    python tests/tools/sobol_timing.py [--B 64] [--n 2000] [--D 10] [--N 65536] [--reps 5] [--out FILE]

Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mogp_emulator_amd as M                                     # noqa: E402
from mogp_emulator_amd import _capi                               # noqa: E402
from mogp_emulator_amd.Priors import GPPriors                     # noqa: E402
from sobol_restate import all_points, sobol_restate, split_points  # noqa: E402

TAGS = ("sobol_pick_freeze", "cross_cov", "sobol_moments", "sobol_reduce")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--N", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not M.gpu_usable():
        raise SystemExit("sobol_timing: no gfx950 device (or the library is not built)")
    lib = _capi.load()
    rng = np.random.default_rng(0)
    X = rng.uniform(0., 1., (a.n, a.D))
    T = np.stack([np.sin(3. * X @ rng.normal(size=a.D)) + 0.01 * rng.normal(size=a.n) for _ in range(a.B)])
    mo = M.MultiOutputGP_GPU(X, T, nugget=1e-6, priors=GPPriors(n_corr=a.D, nugget_type="fixed"))
    mo.fit(np.tile(np.array([1.0] * a.D + [0.0]), (a.B, 1)))
    A, B = rng.uniform(0., 1., (a.N, a.D)), rng.uniform(0., 1., (a.N, a.D))
    box = {}

    def fused():
        box["fused"] = M.sobol_indices(mo, A=A, B=B)

    def existing():
        f = mo.predict(all_points(A, B), unc=False, deriv=False).mean
        box["existing"] = sobol_restate(*split_points(f, a.N, a.D))

    def existing_predict_only():
        box["f"] = mo.predict(box["P"], unc=False, deriv=False).mean

    fused()
    existing()
    tf, te = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); fused(); tf.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); existing(); te.append(time.perf_counter() - t0)
    box["P"] = all_points(A, B)
    tp = []
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter(); existing_predict_only(); tp.append(time.perf_counter() - t0)
    res = {"B": a.B, "n": a.n, "D": a.D, "N": a.N, "reps": a.reps,
           "fused_s": statistics.median(tf), "fused_min_s": min(tf), "fused_max_s": max(tf),
           "existing_s": statistics.median(te), "existing_min_s": min(te), "existing_max_s": max(te),
           "existing_predict_only_s": statistics.median(tp)}
    res["speedup"] = res["existing_s"] / res["fused_s"]
    res["max_abs_diff_S"] = float(np.max(np.abs(box["fused"].first_order - box["existing"]["first_order"])))
    res["max_abs_diff_ST"] = float(np.max(np.abs(box["fused"].total - box["existing"]["total"])))
    # kernels of one fused call, by tag (the events serialise nothing on one stream, but they are a run of their own all the same)
    lib.mogp_profile_reset()
    lib.mogp_profile_enable(1)
    t0 = time.perf_counter()
    fused()
    res["fused_profiled_s"] = time.perf_counter() - t0
    lib.mogp_profile_enable(0)
    for tag in TAGS:
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) != 0:
            raise RuntimeError("no profile record for " + tag)
        res[tag + "_ms"], res[tag + "_launches"], res[tag + "_alg_bytes"] = ms.value, cnt.value, by.value
        res[tag + "_GBps"] = by.value / (ms.value * 1e-3) / 1e9 if ms.value > 0 else 0.

    print("sensitivity analysis, %d emulators x n = %d x D = %d, N = %d (median of %d, min - max):" % (a.B, a.n, a.D, a.N, a.reps))
    print("  sobol_indices (fused)                     %8.4f s   (%.4f - %.4f)" % (res["fused_s"], res["fused_min_s"], res["fused_max_s"]))
    print("  predict of (D + 2) N points + NumPy pass  %8.4f s   (%.4f - %.4f)   -> %.3f x"
          % (res["existing_s"], res["existing_min_s"], res["existing_max_s"], res["speedup"]))
    print("    of which the predict call alone         %8.4f s" % res["existing_predict_only_s"])
    for tag in TAGS:
        print("  kernels %-18s %10.3f ms  %5d launch groups  %8.1f GB/s algorithmic  (%.2f %% of the fused call)"
              % (tag, res[tag + "_ms"], res[tag + "_launches"], res[tag + "_GBps"], 100. * res[tag + "_ms"] * 1e-3 / res["fused_s"]))
    print("  max |S - restatement| %.3g   max |ST - restatement| %.3g" % (res["max_abs_diff_S"], res["max_abs_diff_ST"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ok = res["fused_s"] <= 1.02 * res["existing_s"]
    if not ok:
        print("FAIL: the fused call (%.4f s) is slower than the existing path (%.4f s) by more than 2 %%" % (res["fused_s"], res["existing_s"]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
