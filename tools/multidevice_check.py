"""Cost of spreading one MultiOutputGP_GPU over a device list, against the single engine, in one process:
fit_GP_MAP (64 emulators x n = 2000, 15 starts) and predict (64 x 10^4 points, host buffers, variances included).

On one GPU with --devices 0,0 the two parts run one after the other under the device's mutex, so the multi-part model should cost what
two 32-emulator batches cost, and no more: what remains beyond that is locking and thread overhead.  On a box with two or more GPUs,
--devices all measures the speed-up.  Prints one JSON line; --out FILE writes it there too.

    python tools/multidevice_check.py [--devices 0,0] [--reps 3] [--out profiles/multidevice_check.json]
    env: B (64), N (2000), D (10), M (10000), TRIES (15)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd import LibGPGPU
    from mogp_emulator_amd.devices import parse_devices
    from mogp_emulator_amd.Priors import GPPriors
    from bench import synth
    B, n, d, m, tries = (int(os.environ.get(k, v)) for k, v in (("B", 64), ("N", 2000), ("D", 10), ("M", 10000), ("TRIES", 15)))
    devices = parse_devices(args.devices, LibGPGPU.device_count())
    X, T, Xs = synth(2, n, d, B, m)
    theta = np.array([-2. * np.log(0.3 * np.sqrt(d))] * d + [0.])

    def build(devs, half=False):
        TT = T[: B // 2] if half else T
        return M.MultiOutputGP_GPU(X, TT, nugget=1e-6, priors=GPPriors(n_corr=d, nugget_type="fixed"), devices=devs)

    def time_map(devs, half=False):
        ts, recs = [], []
        for rep in range(args.reps + 1):          # the first call is a warm-up (replica engine allocation)
            LibGPGPU.set_fit_options(seed=7)
            gp = build(devs, half)
            t0 = time.perf_counter()
            M.fit_GP_MAP(gp, n_tries=tries)
            dt = time.perf_counter() - t0
            if rep:
                ts.append(dt)
            recs.append(gp.fit_record())
        return ts, recs

    def counters():
        out = {}
        for name in ("mchol_aborts", "backsolve_timeouts"):
            v = ctypes.c_longlong(0)
            _capi.load().mogp_profile_counter(name.encode(), ctypes.byref(v))
            out[name] = v.value
        return out

    def same(a, b):
        """emulators whose fit status, log-posterior (NaN = NaN) or theta differ between two fit records"""
        bad = []
        for k in range(len(a["fit_ok"])):
            ta, tb = a["theta"][k], b["theta"][k]
            eq = (a["fit_ok"][k] == b["fit_ok"][k] and np.array_equal(a["logpost"][k], b["logpost"][k], equal_nan=True)
                  and ((ta is None and tb is None) or (ta is not None and tb is not None and np.array_equal(ta, tb))))
            if not eq:
                bad.append(k)
        return bad

    def time_predict(devs, half=False):
        gp = build(devs, half)
        gp.fit(np.tile(theta, (gp.n_emulators, 1)))
        gp.predict(Xs, deriv=False)
        ts = []
        for _ in range(max(args.reps, 5)):
            t0 = time.perf_counter()
            r = gp.predict(Xs, deriv=False)
            ts.append(time.perf_counter() - t0)
        return ts, r

    res = {"B": B, "n": n, "D": d, "m": m, "n_tries": tries, "devices": devices, "visible_gpus": LibGPGPU.device_count()}
    c0 = counters()
    single_map, recs1 = time_map(None)
    multi_map, recs2 = time_map(devices)
    half_map, _ = time_map(None, half=True)
    res["fit_GP_MAP_s"] = {"single": single_map, "multi": multi_map, "single_32": half_map}
    # emulators whose result differs: multi-part against single engine, and the single engine against its own previous call
    res["fit_GP_MAP_differ_multi_vs_single"] = same(recs1[-1], recs2[-1])
    res["fit_GP_MAP_differ_single_vs_single"] = same(recs1[-1], recs1[-2])
    res["fit_GP_MAP_not_fit"] = [k for k, ok in enumerate(recs1[-1]["fit_ok"]) if not ok]
    lp1, lp2 = np.array(recs1[-1]["logpost"]), np.array(recs2[-1]["logpost"])
    res["fit_GP_MAP_logpost_max_rel_diff"] = float(np.nanmax(np.abs(lp1 - lp2) / np.maximum(np.abs(lp1), 1e-300)))
    res["counters"] = {k: v - c0[k] for k, v in counters().items()}
    single_pr, r1 = time_predict(None)
    multi_pr, r2 = time_predict(devices)
    half_pr, _ = time_predict(None, half=True)
    res["predict_s"] = {"single": single_pr, "multi": multi_pr, "single_32": half_pr}
    res["predict_mean_identical"] = bool(np.array_equal(r1.mean, r2.mean))
    res["predict_var_maxdiff"] = float(np.max(np.abs(r1.unc - r2.unc)))
    med = lambda v: float(np.median(v))          # noqa: E731
    res["summary"] = {
        "fit_GP_MAP_multi_over_single": med(multi_map) / med(single_map),
        "fit_GP_MAP_multi_over_2x32": med(multi_map) / (2 * med(half_map)),
        "predict_multi_over_single": med(multi_pr) / med(single_pr),
        "predict_multi_over_2x32": med(multi_pr) / (2 * med(half_pr)),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
