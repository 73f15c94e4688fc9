"""One MultiOutputGP_GPU spread over several devices in one process (devices=...): every part is an engine of its own on its
device, and the model computes what the single-engine model computes.  On a one-GPU box the parts share device 0 ([0, 0], [0, 0, 0]):
each part is still its own engine, run on its own host thread under the device's mutex, so the split, the row placement, the start
draws of fit_GP_MAP, the cross-part implausibility merge and the error path are all exercised.  Tests that need two distinct GPUs skip
with a reason elsewhere."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
from mogp_emulator_amd.HistoryMatching import HistoryMatching

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, M_PTS = 90, 3, 37


def _data(ne, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0., 1., (N, D))
    T = np.stack([np.sin(2.5 * X @ rng.normal(size=D)) + 0.3 * k + 0.01 * rng.normal(size=N) for k in range(ne)])
    Xs = rng.uniform(0., 1., (M_PTS, D))
    return X, T, Xs


MODES = {
    "theta_mean": dict(mean="c+c*x[0]"),
    "analytic_mean": dict(mean="c+c*x[0]", analytic_mean=True),
    "pivot": dict(nugget="pivot"),
}


def _thetas(gp, ne):
    npar = gp._mogp_gpu.emulator(0).n_params() + gp._mogp_gpu.emulator(0).get_theta().get_n_mean()
    rows = []
    for k in range(ne):
        nm = npar - (D + 1)
        rows.append(np.concatenate([0.1 * np.arange(1, nm + 1) * (-1) ** k, [-1.2 + 0.1 * k, -0.8, -0.5 + 0.05 * k], [0.2 - 0.03 * k]]))
    return np.array(rows)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("ne", [2, 5, 7])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_fit_and_predict_match_the_single_engine(devices, ne, mode):
    X, T, Xs = _data(ne)
    kw = MODES[mode]
    single = M.MultiOutputGP_GPU(X, T, **kw)
    multi = M.MultiOutputGP_GPU(X, T, devices=devices, **kw)
    per = -(-ne // len(devices))
    want = [(0, lo, min(lo + per, ne)) for lo in range(0, ne, per)]
    assert multi._mogp_gpu.parts() == want
    assert multi.devices == [0] * len(want)
    assert single.devices == [0] and single._mogp_gpu.n_parts() == 1
    th = _thetas(single, ne)
    f1, g1, ok1 = single._mogp_gpu.eval(th, grad=True)
    f2, g2, ok2 = multi._mogp_gpu.eval(th, grad=True)
    assert ok1.all() and ok2.all()
    assert_array_equal(f2, f1)
    assert_array_equal(g2, g1)
    single.fit(th)
    multi.fit(th)
    assert multi.get_indices_fit() == list(range(ne))
    r1 = single.predict(Xs)
    r2 = multi.predict(Xs)
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)
    assert_array_equal(r2.deriv, r1.deriv)
    assert_array_equal(multi.targets, single.targets)
    rec1, rec2 = single.fit_record(), multi.fit_record()
    assert rec2["fit_ok"] == rec1["fit_ok"] and rec2["nugget"] == rec1["nugget"]
    assert_array_equal(rec2["logpost"], rec1["logpost"])


_MAP_SCRIPT = r"""
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
import mogp_emulator_amd as M
from mogp_emulator_amd import LibGPGPU
rng = np.random.default_rng(11)
X = rng.uniform(0., 1., (70, 3))
T = np.stack([np.sin(2. * X @ rng.normal(size=3)) + 0.02 * rng.normal(size=70) for _ in range(5)])
def run(devices):
    LibGPGPU.set_fit_options(seed=1)
    gp = M.MultiOutputGP_GPU(X, T, devices=devices)
    M.fit_GP_MAP(gp, n_tries=3)
    rec = gp.fit_record()
    return {"ok": rec["fit_ok"], "logpost": rec["logpost"], "nugget": rec["nugget"],
            "theta": [None if t is None else [float(v) for v in t] for t in rec["theta"]], "parts": gp._mogp_gpu.n_parts()}
a, b = run(None), run([0, 0, 0])
print("MAP-RESULT " + json.dumps({"single": a, "multi": b}))
"""


@pytest.mark.parametrize("chol", [None, "left"])
def test_fit_GP_MAP_on_three_parts_is_bit_identical(chol):
    """n_tries=3, seed=1: the multi-part fit draws every start where the single engine draws it and ends where it ends, bit for bit
    (float -> JSON -> float is exact).  Each schedule in its own process: the library reads MOGP_CHOL once."""
    env = dict(os.environ)
    env.pop("MOGP_CHOL", None)
    env.pop("MOGP_DEVICES", None)
    if chol:
        env["MOGP_CHOL"] = chol
    out = subprocess.run([sys.executable, "-c", _MAP_SCRIPT % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("MAP-RESULT ")][-1]
    res = json.loads(line[len("MAP-RESULT "):])
    a, b = res["single"], res["multi"]
    assert a["parts"] == 1 and b["parts"] == 3
    assert all(a["ok"])
    assert b["ok"] == a["ok"]
    assert b["logpost"] == a["logpost"]
    assert b["nugget"] == a["nugget"]
    assert b["theta"] == a["theta"]


def test_full_cov_and_rows_of_emulators_not_fit():
    X, T, Xs = _data(7)
    single = M.MultiOutputGP_GPU(X, T)
    multi = M.MultiOutputGP_GPU(X, T, devices=[0, 0, 0])
    th = _thetas(single, 7)
    single.fit(th)
    multi.fit(th)
    r1 = single.predict(Xs[:9], full_cov=True)
    r2 = multi.predict(Xs[:9], full_cov=True)
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)
    # emulators 1 (part 0) and 6 (the last part) not fit
    for gp in (single, multi):
        gp.reset_fit_status()
        for k in (0, 2, 3, 4, 5):
            gp.fit_emulator(k, th[k])
    assert multi.get_indices_not_fit() == [1, 6] == single.get_indices_not_fit()
    with pytest.raises(ValueError):
        multi.predict(Xs)
    r1 = single.predict(Xs, allow_not_fit=True)
    r2 = multi.predict(Xs, allow_not_fit=True)
    assert np.isnan(r2.mean[[1, 6]]).all() and np.isnan(r2.unc[[1, 6]]).all() and np.isnan(r2.deriv[[1, 6]]).all()
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)
    assert_array_equal(r2.deriv, r1.deriv)
    r1 = single.predict(Xs[:5], allow_not_fit=True, full_cov=True)
    r2 = multi.predict(Xs[:5], allow_not_fit=True, full_cov=True)
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)


def test_predict_dev_into_torch_buffers_matches_the_single_engine():
    import torch
    X, T, Xs = _data(7)
    single = M.MultiOutputGP_GPU(X, T, mean="c+c*x[1]")
    multi = M.MultiOutputGP_GPU(X, T, mean="c+c*x[1]", devices=[0, 0, 0])
    th = _thetas(single, 7)
    dev = torch.device("cuda", 0)
    d_xs = torch.from_numpy(Xs).to(dev)

    def run(gp):
        outs = [torch.full(shape, 7.0, dtype=torch.float64, device=dev) for shape in ((7, M_PTS), (7, M_PTS), (7, M_PTS, D))]
        gp._mogp_gpu.predict_dev(d_xs.data_ptr(), M_PTS, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    for gp in (single, multi):
        gp.fit(th)
    a, b = run(single), run(multi)
    assert np.isfinite(b[0]).all()
    assert_array_equal(b[0], a[0])
    assert_allclose(b[1], a[1], rtol=0, atol=1e-15)
    assert_array_equal(b[2], a[2])
    for gp in (single, multi):
        gp.reset_fit_status()
        for k in (0, 1, 2, 4, 5):
            gp.fit_emulator(k, th[k])
    a, b = run(single), run(multi)
    for arr in b:
        assert np.isnan(arr[[3, 6]]).all() and np.isfinite(arr[[0, 1, 2, 4, 5]]).all()
    assert_array_equal(b[0], a[0])
    assert_allclose(b[1], a[1], rtol=0, atol=1e-15)
    assert_array_equal(b[2], a[2])


@pytest.mark.parametrize("rank", [0, 1, 3])
def test_implausibility_over_three_parts(rank):
    X, T, Xs = _data(7)
    single = M.MultiOutputGP_GPU(X, T)
    multi = M.MultiOutputGP_GPU(X, T, devices=[0, 0, 0])
    assert multi._mogp_gpu.n_parts() == 3
    th = _thetas(single, 7)
    single.fit(th)
    multi.fit(th)
    rng = np.random.default_rng(5)
    z = rng.normal(size=7)
    zvar = rng.uniform(0.01, 0.1, 7)
    disc = rng.uniform(0., 0.05, 7)
    I1 = single._mogp_gpu.implausibility(Xs, z, zvar, disc, include_nugget=True, rank=rank)
    I2 = multi._mogp_gpu.implausibility(Xs, z, zvar, disc, include_nugget=True, rank=rank)
    assert_array_equal(I2, I1)
    # the (rank+1)-th largest of the per-emulator implausibilities recomputed from the model's own predict
    r = multi.predict(Xs, deriv=False)
    scores = np.abs(z[:, None] - r.mean) / np.sqrt(r.unc + zvar[:, None] + disc[:, None])
    want = -np.sort(-scores, axis=0)[rank]
    assert_allclose(I2, want, rtol=1e-13)
    h1 = HistoryMatching(gp=single, obs=[z, zvar], coords=Xs).get_implausibility(disc, rank=rank)
    h2 = HistoryMatching(gp=multi, obs=[z, zvar], coords=Xs).get_implausibility(disc, rank=rank)
    assert_array_equal(h2, h1)
    assert_array_equal(h2, I1)


def test_implausibility_of_many_points_chunks_like_the_single_engine():
    """more query points than one chunk of the engines' scratch (7 emulators x n = 90: 6e9 / (7 x 128 x 8) points per chunk is
    far above this; the merge still runs chunk by chunk of its own) -- a large m checked against the single engine"""
    X, T, _ = _data(7)
    Xs = np.random.default_rng(9).uniform(0., 1., (20000, D))
    single = M.MultiOutputGP_GPU(X, T)
    multi = M.MultiOutputGP_GPU(X, T, devices=[0, 0, 0])
    th = _thetas(single, 7)
    single.fit(th)
    multi.fit(th)
    z = np.linspace(-1., 1., 7)
    I1 = single._mogp_gpu.implausibility(Xs, z, 0.05 * np.ones(7), np.zeros(7), rank=2)
    I2 = multi._mogp_gpu.implausibility(Xs, z, 0.05 * np.ones(7), np.zeros(7), rank=2)
    assert_array_equal(I2, I1)


def test_error_in_the_last_part_is_raised_on_the_caller_and_the_handle_stays_usable():
    X, T, Xs = _data(7)
    single = M.MultiOutputGP_GPU(X, T)
    multi = M.MultiOutputGP_GPU(X, T, devices=[0, 0, 0])
    th = _thetas(single, 7)
    single.fit(th)
    multi.fit(th)
    zvar = 0.05 * np.ones(7)
    zvar[6] = -1.
    with pytest.raises(RuntimeError, match="observation variance cannot be negative") as exc:
        multi._mogp_gpu.implausibility(Xs, np.zeros(7), zvar, np.zeros(7), rank=1)
    assert "emulators [6, 7)" in str(exc.value)
    r1, r2 = single.predict(Xs), multi.predict(Xs)
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)
    I1 = single._mogp_gpu.implausibility(Xs, np.zeros(7), 0.05 * np.ones(7), np.zeros(7), rank=1)
    I2 = multi._mogp_gpu.implausibility(Xs, np.zeros(7), 0.05 * np.ones(7), np.zeros(7), rank=1)
    assert_array_equal(I2, I1)


def test_a_handle_built_on_one_thread_is_used_from_another():
    X, T, Xs = _data(5)
    single = M.MultiOutputGP_GPU(X, T)
    th = _thetas(single, 5)
    single.fit(th)
    ref = single.predict(Xs)
    box = {}

    def build():
        box["gp"] = M.MultiOutputGP_GPU(X, T, devices=[0, 0])

    def use():
        try:
            box["gp"].fit(th)
            box["r"] = box["gp"].predict(Xs)
            box["one"] = single.predict(Xs)
        except Exception as e:          # noqa: BLE001 -- re-raised on the test's thread below
            box["err"] = e

    for target in (build, use):
        t = threading.Thread(target=target)
        t.start()
        t.join()
    assert "err" not in box, box.get("err")
    assert_array_equal(box["r"].mean, ref.mean)
    assert_allclose(box["r"].unc, ref.unc, rtol=0, atol=1e-15)
    assert_array_equal(box["one"].mean, ref.mean)


def test_MOGP_DEVICES_spreads_a_model_with_no_code_change():
    script = ("import sys; sys.path.insert(0, %r)\n"
              "import numpy as np, mogp_emulator_amd as M\n"
              "rng = np.random.default_rng(0); X = rng.uniform(0, 1, (40, 2)); T = np.stack([np.sin(3 * X[:, 0] + k) for k in range(3)])\n"
              "gp = M.fit_GP_MAP(X, T, n_tries=1)\n"
              "print('PARTS', gp._mogp_gpu.parts(), gp.devices, gp.get_indices_fit())\n" % ROOT)
    env = dict(os.environ, MOGP_DEVICES="0,0")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "PARTS [(0, 0, 2), (0, 2, 3)] [0, 0] [0, 1, 2]" in out.stdout, out.stdout


def test_fit_GP_MAP_passes_devices_on():
    X, T, _ = _data(4)
    gp = M.fit_GP_MAP(X, T, n_tries=1, devices=[0, 0])
    assert gp.devices == [0, 0] and gp._mogp_gpu.parts() == [(0, 0, 2), (0, 2, 4)]
    assert gp.get_indices_fit() == [0, 1, 2, 3]


def test_out_of_range_ordinal_is_refused():
    X, T, _ = _data(2)
    n = LibGPGPU.device_count()
    with pytest.raises(ValueError, match="out of range"):
        M.MultiOutputGP_GPU(X, T, devices=[0, n])
    with pytest.raises(RuntimeError, match="out of range"):
        LibGPGPU.MultiOutputGP_GPU(X, T, 100, devices=[n])


_NEED_TWO = pytest.mark.skipif(LibGPGPU.device_count() < 2, reason="needs two or more GPUs (unverified on a one-GPU box)")


@_NEED_TWO
def test_device_guard_after_set_device_elsewhere():
    import torch
    X, T, Xs = _data(3)
    torch.cuda.set_device(0)
    gp = M.MultiOutputGP_GPU(X, T)
    th = _thetas(gp, 3)
    gp.fit(th)
    ref = gp.predict(Xs)
    torch.cuda.set_device(1)
    try:
        r = gp.predict(Xs)
        assert torch.cuda.current_device() == 1
    finally:
        torch.cuda.set_device(0)
    assert_array_equal(r.mean, ref.mean)


@_NEED_TWO
def test_all_devices():
    X, T, Xs = _data(7)
    single = M.MultiOutputGP_GPU(X, T)
    multi = M.MultiOutputGP_GPU(X, T, devices="all")
    nd = LibGPGPU.device_count()
    assert sorted(set(multi.devices)) == list(range(min(nd, 7)))
    th = _thetas(single, 7)
    single.fit(th)
    multi.fit(th)
    r1, r2 = single.predict(Xs), multi.predict(Xs)
    assert_array_equal(r2.mean, r1.mean)
    assert_allclose(r2.unc, r1.unc, rtol=0, atol=1e-15)
    z = np.zeros(7)
    assert_array_equal(multi._mogp_gpu.implausibility(Xs, z, 0.1 * np.ones(7), z, rank=2),
                       single._mogp_gpu.implausibility(Xs, z, 0.1 * np.ones(7), z, rank=2))
