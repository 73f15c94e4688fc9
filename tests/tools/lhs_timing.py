"""Times of the Latin-hypercube annealer on one MI355X, median of 5 after one warm-up, as one JSON line and a readable table:

 1. ``design_anneal_lhs`` at n = 2000, D = 10 with 256 chains: the whole call (host arrays in, results out) and the device time of the
    annealing kernel alone (HIP events of the library's profiling registry, tag "design_anneal_lhs"); per proposal and chain, and per
    proposal over all chains;
 2. the minimum distance of the winner against ``MaxiMinLHC`` given the same wall time (as many random tries as fit into it);
 3. the NumPy restatement (tests/lhs_restate.py) on this host, one chain, on a short prefix of the proposals, scaled;
 4. a default ``OptimisedLHC(D).sample(n)`` call, all of it.

    python tests/tools/lhs_timing.py [--n 2000] [--D 10] [--chains 256] [--steps 0] [--reps 5] [--out FILE]

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
import mogp_emulator_amd as M                                                     # noqa: E402
from mogp_emulator_amd import _capi                                               # noqa: E402
from mogp_emulator_amd.ExperimentalDesign import MaxiMinLHC, OptimisedLHC         # noqa: E402
import lhs_restate as lr                                                          # noqa: E402


def median_time(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def kernel_ms(lib, fn, reps):
    got = []
    for _ in range(reps):
        lib.mogp_profile_reset()
        lib.mogp_profile_enable(1)
        fn()
        lib.mogp_profile_enable(0)
        ms, cnt, fl, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        if lib.mogp_profile_get(b"design_anneal_lhs", ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by)) != 0:
            raise RuntimeError("no profile record for design_anneal_lhs")
        got.append(ms.value)
    return statistics.median(got)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=0, help="proposals per chain (0 = the default of OptimisedLHC)")
    ap.add_argument("--host-steps", type=int, default=200, help="proposals of the restatement that are timed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-default-call", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not M.gpu_usable():
        raise SystemExit("lhs_timing: no gfx950 device (or the library is not built)")
    from mogp_emulator_amd import libgpgpu
    lib = _capi.load()
    n, D, C = a.n, a.D, a.chains
    steps = a.steps or OptimisedLHC.STEPS_PER_CELL * n * D
    res = {"n": n, "D": D, "chains": C, "steps": steps, "reps": a.reps}
    rng = np.random.default_rng(2024)
    S = np.stack([np.stack([rng.permutation(n) for _ in range(D)], axis=1) for _ in range(C)]).astype(np.int32)
    out = {}

    def device():
        out["r"] = libgpgpu.design_anneal_lhs(S, steps, seed=7)
    res["call_s"] = median_time(device, a.reps)
    res["kernel_s"] = kernel_ms(lib, device, a.reps) * 1e-3
    res["us_per_proposal_per_chain"] = res["kernel_s"] / steps * 1e6
    res["us_per_proposal_all_chains"] = res["kernel_s"] / steps / C * 1e6
    r = out["r"]
    w = r.winner
    res["winner_min_r"], res["winner_pairs"], res["start_min_r_best"] = int(r.min_r[w]), int(r.pairs[w]), int(max(lr.criteria(s)[0] for s in S[:8]))
    res["chains_min_r_range"] = [int(r.min_r.min()), int(r.min_r.max())]
    res["accepted_share"] = float(r.accepted.mean() / max(steps, 1))
    res["winner_min_dist"] = float(libgpgpu.design_min_pdist((r.levels[w] + 0.5) / n)[0])

    # MaxiMinLHC with the same wall time: as many tries as one second of it draws and scores, scaled
    mm = MaxiMinLHC(D)
    np.random.seed(3)
    t0 = time.perf_counter()
    mm._draw_samples(n, n_tries=200)
    per_try = (time.perf_counter() - t0) / 200
    tries = max(1, int(res["call_s"] / per_try))
    np.random.seed(3)
    t0 = time.perf_counter()
    best = mm._draw_samples(n, n_tries=tries)
    res["maximin_tries"], res["maximin_s"] = tries, time.perf_counter() - t0
    res["maximin_min_dist"] = float(libgpgpu.design_min_pdist(best)[0])

    # the restatement on this host: one chain, a short prefix
    t0 = time.perf_counter()
    lr.anneal(S[0], 0)
    base = time.perf_counter() - t0
    t0 = time.perf_counter()
    lr.anneal(S[0], a.host_steps)
    res["host_us_per_proposal"] = (time.perf_counter() - t0 - base) / a.host_steps * 1e6
    res["speedup_per_chain"] = res["host_us_per_proposal"] / res["us_per_proposal_per_chain"]
    res["speedup_all_chains"] = res["host_us_per_proposal"] / res["us_per_proposal_all_chains"]

    if not a.skip_default_call:
        def default_call():
            np.random.seed(5)
            OptimisedLHC(D).sample(n)
        res["default_sample_s"] = median_time(default_call, max(1, min(a.reps, 3)))

    print("design_anneal_lhs, n = %d, D = %d, %d chains of %d proposals (median of %d):" % (n, D, C, steps, a.reps))
    print("  the call, host arrays in, results out   %9.4f s" % res["call_s"])
    print("  the annealing kernel alone              %9.4f s   = %.3f us per proposal and chain, %.5f us per proposal over all chains"
          % (res["kernel_s"], res["us_per_proposal_per_chain"], res["us_per_proposal_all_chains"]))
    print("  accepted share %.3f; min R of the chains %s, winner %d with %d pair(s); best of 8 starts %d"
          % (res["accepted_share"], res["chains_min_r_range"], res["winner_min_r"], res["winner_pairs"], res["start_min_r_best"]))
    print("  minimum distance: annealed %.5f, MaxiMinLHC of %d tries in %.3f s %.5f"
          % (res["winner_min_dist"], tries, res["maximin_s"], res["maximin_min_dist"]))
    print("  NumPy restatement on this host          %9.1f us per proposal (one chain)  -> %.0f x per chain, %.0f x over all chains"
          % (res["host_us_per_proposal"], res["speedup_per_chain"], res["speedup_all_chains"]))
    if "default_sample_s" in res:
        print("  OptimisedLHC(%d).sample(%d), defaults     %9.4f s" % (D, n, res["default_sample_s"]))
    ok = res["winner_min_dist"] > res["maximin_min_dist"]
    if not ok:
        print("FAIL: the annealed design is not better than MaxiMinLHC at equal wall time")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
