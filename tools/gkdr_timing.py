"""Wall time of gKDR's device call (libgpgpu.gkdr_R) on the grid a tuning search makes: 3 x 3 (X_scale, Y_scale) pairs at N = 2000
and 5000 with M = 10, and one pair at N = 200, M = 3200.  One JSON line per configuration: median / min of the timed calls (ms,
host wall clock around the whole call: uploads, every kernel, the download of R) and the achieved fp64 rate of the algorithmic
flops (per input scale: Kx Kx 2 N^3, Cholesky N^3 / 3, L^-1 N^3 / 3; per pair: four triangular-times-full products 4 N^3, F Kx
2 N^3 and the sandwiches 2 N^2 M + 2 N M^2).

    python tools/gkdr_timing.py [--reps 10] [--only N,M]     (--only: one configuration, e.g. for a profile of its own)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mogp_emulator_amd import LibGPGPU  # noqa: E402
from mogp_emulator_amd.DimensionReduction import median_dist  # noqa: E402


def flops(n, m, nx, ny):
    return nx * (2 + 2.0 / 3) * n ** 3 + nx * ny * (6.0 * n ** 3 + 2.0 * n * n * m + 2.0 * n * m * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    assert LibGPGPU.gpu_usable(), "no gfx950 device"
    rng = np.random.default_rng(0)
    for n, m, cx, cy in [(2000, 10, (0.5, 1.0, 5.0), (0.5, 1.0, 5.0)), (5000, 10, (0.5, 1.0, 5.0), (0.5, 1.0, 5.0)),
                         (200, 3200, (1.0,), (1.0,))]:
        if a.only and a.only != "%d,%d" % (n, m):
            continue
        X = rng.uniform(0, 1, (n, m))
        Y = np.sin(X[:, 0] + 2 * X[:, 1]) + 0.01 * rng.normal(size=n)
        mx, my = median_dist(X), median_dist(Y[:, None])
        sx = [(c * mx) ** 2 for c in cx]
        sy = [(c * my) ** 2 for c in cy]
        LibGPGPU.gkdr_R(X, Y, sx, sy, 1e-8)            # warm-up: code objects, allocator
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            R, info = LibGPGPU.gkdr_R(X, Y, sx, sy, 1e-8)
            ts.append(time.perf_counter() - t0)
        assert not info.any() and np.all(np.isfinite(R))
        med = float(np.median(ts))
        fl = flops(n, m, len(sx), len(sy))
        print(json.dumps({"n": n, "m": m, "pairs": len(sx) * len(sy), "median_ms": round(med * 1e3, 3),
                          "min_ms": round(min(ts) * 1e3, 3), "gflop": round(fl / 1e9, 2),
                          "tflops_at_median": round(fl / med / 1e12, 2)}), flush=True)


if __name__ == "__main__":
    main()
