"""Times of the iterative exact likelihood (IterativeGP.log_likelihood, VecchiaGP.loglik_exact / fit_exact) on one MI355X, as JSON lines.
Squared exponential, D = 10, the data and the theta of tests/tools/iterative_timing.py.  DESIGN.md section 3 "Iterative exact likelihood" has
the measured table (the fit at N = 10^5 has not been run).

 eval   N design points (10^5, then 16 000), p = 1024 and 256, 15 probes, rtol 1e-8:
          precondition   the build of the preconditioner (rank reached, wall time)
          value          one ``loglik_exact`` without the gradient: wall time, iterations per column, log|A| and its standard error
          gradient       the same with ``grad=True``; ``sweep_ms`` the HIP-event time of kgrad_forms alone, ``kmatvec_ms`` of one product --
                         the expectation to hold it against is a sweep of the order of one product at D = 10, and an evaluation of about 83
                         products of 29 ms behind the 0.30 s preconditioner at N = 10^5, p = 1024
 fit    ``VecchiaGP.fit`` (k = 30) and then ``fit_exact`` from its optimum: wall time and evaluations of each; at N = 16 000 also the DENSE
        log-likelihood at both optima, which says what the exact fit gained: ``-current_logpost`` of a ``GaussianProcessGPU`` fitted at that
        theta (``current_logpost`` is the NEGATIVE log-posterior; with ``GPPriors(n_corr=D, nugget_type="fit")`` every prior is weak, so it is
        the negative log-likelihood).

    python tests/tools/exact_lik_timing.py [--N 100000] [--D 10] [--limit 1100]

Every step is a child process under its own ``timeout``; a step that fails, or runs out of time, ends the run (nothing further is started
on the device).  Fails without a GPU: a time taken anywhere else says nothing."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from iterative_timing import MAX_ITER, RTOL, data, kernel_ms, note, wall      # noqa: E402

PROBES = 15


def theta_of(D):
    return np.concatenate([np.log(1. / D) + np.linspace(1., 3., D), [0.1, -6.]])


def step_eval(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd import _capi
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    lib = _capi.load()
    N, D = args.N, args.D
    X, t, _ = data(N, D, 1)
    theta = theta_of(D)
    vg = M.VecchiaGP(X, t, n_neighbours=30, nugget="fit", order=np.arange(N))
    out = {"step": "eval", "N": N, "D": D, "probes": PROBES, "rtol": RTOL}
    for p in (1024, 256):
        kw = dict(n_probes=PROBES, precond_rank=p, rtol=RTOL, max_iter=MAX_ITER)
        view = vg.exact_view(theta, precond_rank=p)
        s_pre, _ = wall(lambda: view._native.precondition(*view._hyper[0][:4], p))
        s_val, ll = wall(lambda: vg.loglik_exact(theta, **kw))
        s_grad, lg = wall(lambda: vg.loglik_exact(theta, grad=True, **kw))
        out["p%d" % p] = {"precondition_s": s_pre, "rank": int(ll.precond_rank), "value_s": s_val, "gradient_s": s_grad, "ok": bool(ll.ok),
                          "iterations": ll.iterations.tolist(), "logdet": float(ll.logdet), "logdet_se": float(ll.logdet_se),
                          "value": float(ll.value), "grad": None if lg.grad is None else lg.grad.tolist(),
                          "sweep_ms": kernel_ms(lib, lambda: vg.loglik_exact(theta, grad=True, **kw), "kgrad_forms", 1),
                          "kmatvec_ms": kernel_ms(lib, lambda: vg.loglik_exact(theta, **kw), "kmatvec", 1)}
        note("p%d" % p, out["p%d" % p])
    vg.close()
    print(json.dumps(out))


def step_fit(args):
    import mogp_emulator_amd as M
    from mogp_emulator_amd.Priors import GPPriors
    if not M.gpu_usable():
        raise SystemExit("no gfx950 device")
    N, D = args.N, args.D
    X, t, _ = data(N, D, 1)
    vg = M.VecchiaGP(X, t, n_neighbours=30, nugget="fit", rng=0)
    s_v, fv = wall(lambda: vg.fit(theta0=theta_of(D)))
    theta_v = fv.theta.copy()
    s_e, fe = wall(lambda: vg.fit_exact(theta0=theta_v, n_probes=PROBES, precond_rank=min(1024, N), rtol=RTOL, max_iter=MAX_ITER))
    vg.close()
    out = {"step": "fit", "N": N, "D": D,
           "vecchia": {"fit_s": s_v, "evaluations": int(fv.n_evaluations), "converged": bool(fv.converged), "theta": theta_v.tolist()},
           "exact": {"fit_s": s_e, "evaluations": int(fe.n_evaluations), "converged": bool(fe.converged), "theta": fe.theta.tolist(),
                     "value": float(fe.value)}}
    if N <= 16000:                                                          # the dense log-likelihood at both optima (weak priors)
        gp = M.GaussianProcessGPU(X, t, nugget="fit", priors=GPPriors(n_corr=D, nugget_type="fit"))
        for name, th in (("vecchia", theta_v), ("exact", fe.theta)):
            gp.fit(th)
            out[name]["dense_loglik"] = -float(gp.current_logpost)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--limit", type=int, default=1100, help="seconds per step")
    ap.add_argument("--step", choices=["eval", "fit"], default=None)
    args = ap.parse_args()
    if args.step == "eval":
        return step_eval(args)
    if args.step == "fit":
        return step_fit(args)
    base = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--D", str(args.D)]
    sizes = [args.N] + ([16000] if args.N != 16000 else [])
    for name in ("eval", "fit"):
        for N in sizes:
            rc = subprocess.run(base + ["--step", name, "--N", str(N)]).returncode
            if rc != 0:
                raise SystemExit("step %s at N = %d ended with status %d: nothing further is started" % (name, N, rc))


if __name__ == "__main__":
    main()
