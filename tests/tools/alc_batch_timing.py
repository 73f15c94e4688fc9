"""Times of a greedy ALC batch on one MI355X, median of --reps (after one warm-up), as JSON lines:

 single  one n = 2000 x D = 10 emulator, m_c = 5000 candidates, m_r = 10^4 reference points, q = 16 picks: one ``alc_batch`` call
         (``select="each"``, scores not kept; and with the scores kept; and ``select="total"``) against what the same build offers without it --
           refit     q x (a new emulator on the design with the picks so far appended, ``fit(theta)``, ``alc_criterion``)
           criterion q x ``alc_criterion`` alone (no conditioning at all: the lower bound of any route that scores with it)
 batch   16 emulators, the same.

Beside it the HIP-event times of the kernels of one call (tags alc_cross and alc_condition), and alc_condition against the bytes it reads:
8 (n16 + t)(MP + 1) bytes per slot, set and step, at the 6.3 TB/s a streaming kernel reaches on this chip.

    python tests/tools/alc_batch_timing.py [--n 2000] [--D 10] [--batch 16] [--mc 5000] [--mr 10000] [--q 16] [--reps 5] [--limit 600]

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
HBM_ACHIEVABLE = 6.3e12


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
        if lib.mogp_profile_get(tag.encode(), ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) == 0 and ms.value > 0:
            out[tag] = {"ms": ms.value, "launches": cnt.value, "tflops": fl.value / ms.value * 1e-9, "gbytes": by.value * 1e-9,
                        "tbytes_per_s": by.value / ms.value * 1e-9}
    return out


def step(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    rng = np.random.default_rng(1)
    n, D, mc, mr, q = args.n, args.D, args.mc, args.mr, args.q
    B = args.batch if args.step == "batch" else 1
    X = rng.random((n, D))
    T = np.array([np.sin(X @ rng.normal(size=D)) + 0.05 * rng.standard_normal(n) for _ in range(B)])
    cand, ref = rng.random((mc, D)), rng.random((mr, D))
    hat = np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -4.]])
    pri = GPPriors(n_corr=D, nugget_type="fit")

    def make(Xd, Td):
        if B > 1:
            gp = M.MultiOutputGP_GPU(Xd, Td, nugget="fit", priors=pri)
            gp.fit(np.tile(hat, (B, 1)))
        else:
            gp = M.GaussianProcessGPU(Xd, Td[0], nugget="fit", priors=pri)
            gp.fit(hat)
        return gp
    gp = make(X, T)
    each = lambda: M.alc_batch(gp, cand, ref, q, keep_scores=False)                   # noqa: E731
    t_b, all_b, res = median_time(each, args.reps)
    t_k, all_k, _ = median_time(lambda: M.alc_batch(gp, cand, ref, q), args.reps)
    t_t, all_t, tot = median_time(lambda: M.alc_batch(gp, cand, ref, q, select="total", keep_scores=False), args.reps)
    t_1, all_1, _ = median_time(lambda: M.alc_batch(gp, cand, ref, 1, keep_scores=False), args.reps)

    def criterion():
        for _ in range(q):
            out = M.alc_criterion(gp, cand, ref)
        return out
    t_c, all_c, _ = median_time(criterion, args.reps)
    picks = tot.picks           # one point per step for every emulator, so that the refitted design is one design

    def refit():
        Xd, Td = X, T
        for i in range(q):
            g = make(Xd, Td)
            out = M.alc_criterion(g, cand, ref)
            Xd, Td = np.vstack([Xd, cand[picks[i]][None, :]]), np.hstack([Td, np.zeros((B, 1))])
        return out
    t_r, all_r, _ = median_time(refit, args.reps)
    out = {"step": args.step, "n": n, "D": D, "emulators": B, "m_c": mc, "m_r": mr, "q": q, "n_picked": res.n_picked.tolist(),
           "alc_batch_s": t_b, "alc_batch_all_s": all_b, "alc_batch_keep_scores_s": t_k, "alc_batch_keep_scores_all_s": all_k,
           "alc_batch_total_s": t_t, "alc_batch_total_all_s": all_t, "alc_batch_q1_s": t_1, "alc_batch_q1_all_s": all_1,
           "per_pick_s": (t_b - t_1) / (q - 1) if q > 1 else None,
           "q_criterion_s": t_c, "q_criterion_all_s": all_c, "one_criterion_s": t_c / q, "q_refit_criterion_s": t_r, "q_refit_criterion_all_s": all_r,
           "ratio_criterion": t_c / t_b, "ratio_refit": t_r / t_b, "batch_removes_of_iv0": (res.total_reduction / res.integrated_variance[:, 0]).tolist()}
    k = kernel_ms(lib, each, ("alc_cross", "alc_condition", "cross_cov", "predict_var"))
    if "alc_condition" in k:
        c = k["alc_condition"]
        c["ms_at_6.3_TB_per_s"] = c["gbytes"] * 1e9 / HBM_ACHIEVABLE * 1e3
        c["fraction_of_achievable"] = c["ms_at_6.3_TB_per_s"] / c["ms"]
    out["kernels"] = k
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--mc", type=int, default=5000)
    ap.add_argument("--mr", type=int, default=10000)
    ap.add_argument("--q", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--step", choices=["batch", "single"], default=None)
    args = ap.parse_args()
    if args.step:
        return step(args)
    for name in ("single", "batch"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", name, "--n", str(args.n),
               "--D", str(args.D), "--batch", str(args.batch), "--mc", str(args.mc), "--mr", str(args.mr), "--q", str(args.q),
               "--reps", str(args.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("step %s ended with status %d: nothing further is started" % (name, rc))


if __name__ == "__main__":
    main()
