"""Times of the design classes on one MI355X, median of 5 (after one warm-up each), as one JSON line and a readable table:

 1. the scoring step of MaxiMinLHC at n = 2000, D = 10, n_tries = 1000: ``design_min_pdist`` on host arrays (host -> device copy included),
    and the device time of its kernels alone (HIP events of the library's profiling registry, tag "design_min_pdist");
 2. the same 1000 ``pdist(...).min()`` calls with scipy on this host -- the reference's own arithmetic, the baseline;
 3. the host-side drawing of the 1000 hypercubes, which neither path can avoid (it bounds the end-to-end gain), and a whole
    ``MaxiMinLHC._draw_samples`` call;
 4. one MICEDesign step (fit_GP_MAP + scoring of all candidates) at 200 design points with n_cand = 50 and n_cand = 5000, and the
    scoring part alone.

    python tests/tools/design_timing.py [--tries 1000] [--n 2000] [--D 10] [--reps 5] [--out FILE]

Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
from scipy.spatial.distance import pdist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import mogp_emulator_amd as M                                                     # noqa: E402
from mogp_emulator_amd import _capi                                               # noqa: E402
from mogp_emulator_amd.ExperimentalDesign import LatinHypercubeDesign, MaxiMinLHC  # noqa: E402


def median_time(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def kernel_ms(lib, fn, reps):
    """Median device time (ms) of the tagged launches of one call of fn."""
    got = []
    for _ in range(reps):
        lib.mogp_profile_reset()
        lib.mogp_profile_enable(1)
        fn()
        lib.mogp_profile_enable(0)
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(b"design_min_pdist", ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) != 0:
            raise RuntimeError("no profile record for design_min_pdist")
        got.append((ms.value, cnt.value, fl.value, by.value))
    got.sort()
    return got[len(got) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=1000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-tries", type=int, default=0, help="tries timed with scipy (0 = all of them)")
    ap.add_argument("--mice-n", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not M.gpu_usable():
        raise SystemExit("design_timing: no gfx950 device (or the library is not built)")
    from mogp_emulator_amd import libgpgpu
    from mogp_emulator_amd.SequentialDesign import MICEDesign
    lib = _capi.load()
    res = {"n": a.n, "D": a.D, "tries": a.tries, "reps": a.reps}

    # the tries, drawn as MaxiMinLHC draws them
    np.random.seed(2024)
    lhc = LatinHypercubeDesign(a.D)
    tries = np.empty((a.tries, a.n, a.D))

    def draw():
        for t in range(a.tries):
            lhc._draw_into(tries[t])
    res["draw_s"], _ = median_time(draw, a.reps)

    # 1. device scoring, copy included; kernels alone
    out = {}

    def device():
        out["d"] = libgpgpu.design_min_pdist(tries)
    res["device_s"], res["device_all_s"] = median_time(device, a.reps)
    # the shim's check that the designs are finite is part of that call: its share
    res["finite_scan_s"], _ = median_time(lambda: bool(np.all(np.isfinite(tries))), a.reps)
    per_pass = max(1, (64 << 20) // (8 * a.n * a.D))                    # DESIGN_SCRATCH_BYTES of engine.h
    res["passes"] = [min(per_pass, a.tries - t0) for t0 in range(0, a.tries, per_pass)]
    ms, launches, flops, nbytes = kernel_ms(lib, device, a.reps)
    res["kernel_ms"], res["kernel_launch_groups"] = ms, launches
    assert launches == len(res["passes"]), "the library's passes differ from this tool's arithmetic"
    res["kernel_alg_flops"], res["kernel_alg_bytes"] = flops, nbytes
    res["kernel_tflops"] = flops / (ms * 1e-3) / 1e12
    # vector fp64: 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz, one operation per lane and instruction (no FMA in this sum)
    peak = 256 * 4 * 16 * 2.4e9
    res["kernel_share_of_valu_issue"] = flops / (ms * 1e-3) / peak

    # 2. scipy on this host
    ns = a.scipy_tries or a.tries
    ref = np.empty(ns)

    def host():
        for t in range(ns):
            ref[t] = pdist(tries[t]).min()
    t_host, _ = median_time(host, a.reps if ns < a.tries else max(1, min(a.reps, 3)))
    res["scipy_tries_timed"] = ns
    res["scipy_s"] = t_host * a.tries / ns
    rtol = 2.0 * (a.D + 2) * 2.0 ** -53
    res["max_rel_diff_vs_scipy"] = float(np.max(np.abs(out["d"][:ns] - ref) / ref))
    assert res["max_rel_diff_vs_scipy"] <= rtol, "device and scipy distances differ by more than the bound"
    assert int(np.argmax(out["d"][:ns])) == int(np.argmax(ref))
    res["speedup_scoring"] = res["scipy_s"] / res["device_s"]

    # 3. a whole maximin draw
    mm = MaxiMinLHC(a.D)

    def whole():
        np.random.seed(7)
        mm._draw_samples(a.n, n_tries=a.tries)
    res["maximin_draw_samples_s"], _ = median_time(whole, a.reps)

    # 4. one MICE step
    def f(x):
        return np.sin(3. * x[0]) + x[1] * x[1] - 0.5 * x[-1]
    for n_cand in (50, 5000):
        np.random.seed(11)
        md = MICEDesign(LatinHypercubeDesign(4), f=f, n_init=a.mice_n, n_cand=n_cand, nugget=1.e-6)
        md.run_initial_design()
        md._generate_candidates()

        def step():
            np.random.seed(13)
            md._eval_metric()
        res["mice_step_s_ncand%d" % n_cand], _ = median_time(step, a.reps)
        res["mice_score_s_ncand%d" % n_cand], _ = median_time(md._score_candidates, a.reps)

    if res["device_s"] >= res["scipy_s"]:
        print("FAIL: device scoring (%.4f s) is not faster than scipy (%.4f s)" % (res["device_s"], res["scipy_s"]))
    print("maximin scoring, %d tries of n = %d, D = %d (median of %d):" % (a.tries, a.n, a.D, a.reps))
    print("  device, host arrays in, distances out   %9.4f s" % res["device_s"])
    print("  of which the finiteness scan on the host %8.4f s   (%.0f %% of the call); passes of %s tries"
          % (res["finite_scan_s"], 100 * res["finite_scan_s"] / res["device_s"], " / ".join(str(k) for k in res["passes"])))
    print("  its kernels alone                       %9.4f s   (%.2f TFLOP/s fp64 of subtract, multiply, add = %.0f %% of vector issue)"
          % (res["kernel_ms"] * 1e-3, res["kernel_tflops"], 100 * res["kernel_share_of_valu_issue"]))
    print("  scipy pdist(...).min() on this host     %9.4f s   (%d tries timed)   -> %.0f x" % (res["scipy_s"], ns, res["speedup_scoring"]))
    print("  drawing the tries on the host           %9.4f s" % res["draw_s"])
    print("  MaxiMinLHC._draw_samples, all of it     %9.4f s" % res["maximin_draw_samples_s"])
    for n_cand in (50, 5000):
        print("MICE step, %d design points, n_cand = %4d:  %9.4f s   (scoring alone %.4f s)"
              % (a.mice_n, n_cand, res["mice_step_s_ncand%d" % n_cand], res["mice_score_s_ncand%d" % n_cand]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["device_s"] < res["scipy_s"] else 1


if __name__ == "__main__":
    sys.exit(main())
