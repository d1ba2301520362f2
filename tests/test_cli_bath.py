"""`nbco3 -bath` and `nbco -bath` on the GPU: the snapshots are those of the same run through Engine.integrate_steps_t / integrate_steps_t_2d,
bit for bit; `nbco3_dist -bath` is refused.  (The argument errors and `nbco3 -cpu -bath` are in tests/test_bath_host.py.)"""
import os
import subprocess

import numpy as np
import pytest

import fmm2d_numpy as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
BATH = ("400", "0", "1500", "2e-6", "1", "0")       # gamma ds = 0.2, 0, 0.75
OMEGA = ("300", "-200", "700")
SEED = 81985529216486895


@pytest.fixture(scope="module")
def host(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return HOST


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["leapfrog", "pefrl_field"])
def test_nbco3_snapshots_are_the_engine_run(host, oracle32, tmp_path, variant):
    """`nbco3 -n 8192 -p 4 -iters 8 -steps 4 -bath ..`: runs of 1, 3, 1, 3, 1 steps (the runs of 3 go through the fused pass), the tick of a
    run its first iteration; every snapshot equals the state of one Engine after as many steps.  The second variant adds -B."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG, INTEG_PEFRL
    n = 8192
    extra, scheme, om = ([], INTEG_LEAPFROG, None) if variant == "leapfrog" else (["-integ", "pefrl", "-B", *OMEGA], INTEG_PEFRL, tuple(float(w) for w in OMEGA))
    r = run(os.path.join(host, "nbco3"), "-n", n, "-p", 4, "-iters", 8, "-steps", 4, "-bath", *BATH, "-bath-seed", SEED, "-o", tmp_path, *extra)
    assert r.returncode == 0, r.stderr
    assert "-bath 400 0 1500 2e-6 1 0" in (tmp_path / "args.txt").read_text()
    gamma, kT = tuple(float(q) for q in BATH[:3]), tuple(float(q) for q in BATH[3:])
    dt = float(np.float32(5e-4))
    e = Engine(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, sync=0)
    d = torch.from_numpy(oracle32.init_reference(n).copy()).cuda().reshape(-1)
    prm = torch.from_numpy(oracle32.params(n)).cuda()
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    done = 0
    for snap in (0, 4, 8):
        e.integrate_steps_t(scheme, EVAL_FMM_KDTREE, d, n, prm, dt, snap + 1 - done, gamma, kT, done, seed=SEED, omega=om)
        done = snap + 1
        e.sync()
        got = np.fromfile(tmp_path / ("out%d_0.000500.bin" % snap), dtype=np.float32)
        assert got.size == 6 * n and got.tobytes() == d[:6 * n].cpu().numpy().tobytes(), snap
    # the bath is in the run: without the flag the last snapshot differs
    plain = tmp_path / "plain"
    plain.mkdir()
    r = run(os.path.join(host, "nbco3"), "-n", n, "-p", 4, "-iters", 8, "-steps", 4, "-o", plain, *extra)
    assert r.returncode == 0, r.stderr
    assert np.fromfile(plain / "out8_0.000500.bin", dtype=np.float32).tobytes() != got.tobytes()
    e.close()


@pytest.mark.gpu
def test_nbco_snapshots_are_the_engine_run(host, tmp_path):
    import torch
    from coulomb_oscillators_amd import Engine, EVAL2D_FMM, INTEG_LEAPFROG, init2d
    n, gamma, kT = 4096, (400.0, 1500.0), (3e-4, 0.0)
    r = run(os.path.join(host, "nbco"), "-n", n, "-iters", 5, "-steps", 2, "-bath", "400", "1500", "3e-4", "0", "-bath-seed", SEED, "-o", tmp_path)
    assert r.returncode == 0, r.stderr
    assert "-bath 400 1500 3e-4 0" in (tmp_path / "args.txt").read_text()
    A, om, xi, om0 = F.kv_params()
    state = init2d(n, "kv", A, om)
    eng = Engine(fmm_order=5, tree_radius=1.0, eps2=float(np.float32(1e-18)), coll=1, dens_inhom=1.0, tree_L=0)
    buf = torch.from_numpy(np.concatenate([state.reshape(-1), np.zeros(2 * n)])).cuda()
    prm = torch.from_numpy(np.array([xi / n, 0.0, om0[0] * om0[0], om0[1] * om0[1]])).cuda()
    eng.compute_force_2d(EVAL2D_FMM, buf, n, prm, elastic=True)
    eng.integrate_steps_t_2d(INTEG_LEAPFROG, EVAL2D_FMM, buf, n, prm, 5e-4, 5, gamma, kT, 0, seed=SEED)
    want = buf[:4 * n].cpu().numpy()
    got = np.fromfile(tmp_path / "out4_0.000500.bin", dtype=np.float64)
    assert np.array_equal(got, want)
    eng.close()
    plain = tmp_path / "plain"
    plain.mkdir()
    r = run(os.path.join(host, "nbco"), "-n", n, "-iters", 5, "-steps", 2, "-o", plain)
    assert r.returncode == 0, r.stderr
    assert not np.array_equal(np.fromfile(plain / "out4_0.000500.bin", dtype=np.float64), got)


def test_nbco3_dist_refuses_the_flag(host):
    r = run(os.path.join(host, "nbco3_dist"), "-gpus", 2, "-bath", 1, 1, 1, 1, 1, 1)
    assert r.returncode != 0 and "'-bath' is not available with kd-domain sharding" in r.stderr and "nbco3 serves it" in r.stderr
