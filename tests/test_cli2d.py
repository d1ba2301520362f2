"""The `nbco` host (the reference's 2-D program main.cu): argument handling without a GPU, snapshots and -test on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import fmm2d_numpy as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBCO = os.path.join(ROOT, "coulomb_oscillators_amd", "host", "nbco")


@pytest.fixture(scope="module")
def nbco(engine_lib):
    if not os.path.exists(NBCO):
        subprocess.check_call(["make", "-C", os.path.dirname(NBCO), "-s", "nbco"])
    return NBCO


def run(exe, *args, cwd=None, timeout=600):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, timeout=timeout)


def test_help(nbco):
    r = run(nbco, "-h")
    assert r.returncode == 0 and "Usage: nbco [options] [input]" in r.stdout
    assert run(nbco, "-help").returncode == 0


@pytest.mark.parametrize("args,msg", [
    (["-n", "0"], "Error: invalid argument to '-n': 0"),
    (["-n"], "Error: missing argument to '-n'"),
    (["-ds", "-1"], "Error: invalid argument to '-ds': -1"),
    (["-iters", "-5"], "Error: invalid argument to '-iters': -5"),
    (["-steps", "0"], "Error: invalid argument to '-steps': 0"),
    (["-integ", "eu"], "Error: invalid argument to '-integ': eu"),
    (["-p", "0"], "Error: invalid argument to '-p': 0"),
    (["-p", "11"], "Error: invalid argument to '-p': 11"),
    (["-r", "0"], "Error: invalid argument to '-r': 0"),
    (["-eps", "0"], "Error: invalid argument to '-eps': 0"),
    (["-eps", "1e-200"], "Error: too small argument to '-eps': 1e-200"),
    (["-i", "0"], "Error: invalid argument to '-i': 0 (should be greater than 0)"),
    (["-gpu", "0"], "Error: invalid argument to '-gpu': 0"),
    (["-gridsize", "x"], "Error: invalid argument to '-gridsize': x"),
    (["-cacheline", "-64"], "Error: invalid argument to '-cacheline': -64"),
    (["-cpu-threads", "0"], "Error: invalid argument to '-cpu-threads': 0"),
    (["-xi", "-1"], "Error: invalid argument to '-xi': -1"),
    (["-omega0", "1"], "Error: missing argument(s) to '-omega0'"),
    (["-A", "1", "-1"], "Error: invalid argument(s) to '-A': 1 -1"),
    (["-bogus"], "Error: unrecognised option '-bogus'"),
    (["-cpu"], "Error: '-cpu' is not available"),
    (["-cpu-threads", "4"], "Error: '-cpu' is not available"),
])
def test_argument_errors(nbco, args, msg):
    r = run(nbco, *args)
    assert r.returncode == 255, (r.returncode, r.stderr)
    assert r.stderr.startswith(msg), r.stderr


def test_missing_input_file(nbco, tmp_path):
    r = run(nbco, str(tmp_path / "absent.bin"))
    assert r.returncode == 255 and "cannot read from input location" in r.stderr


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
def _engine_run(state, n, steps, xi, om0):
    """the library driven as main.cu drives it: one evaluation, then `steps` leapfrog steps (FMM p = 5 + elastic term)"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL2D_FMM, INTEG_LEAPFROG
    eng = Engine(fmm_order=5, tree_radius=1.0, eps2=float(np.float32(1e-18)), coll=1, dens_inhom=1.0, tree_L=0)
    buf = torch.from_numpy(np.concatenate([state.reshape(-1), np.zeros(2 * n)])).cuda()
    prm = torch.from_numpy(np.array([xi / n, 0.0, om0[0] * om0[0], om0[1] * om0[1]])).cuda()
    eng.compute_force_2d(EVAL2D_FMM, buf, n, prm, elastic=True)
    for _ in range(steps):
        eng.integrate_2d(INTEG_LEAPFROG, EVAL2D_FMM, buf, n, prm, 5e-4)
    out = buf[:4 * n].cpu().numpy()
    eng.close()
    return out


@pytest.mark.gpu
def test_snapshots_match_the_engine(nbco, tmp_path):
    from coulomb_oscillators_amd import init2d
    n = 4096
    r = run(nbco, "-n", n, "-iters", 5, "-steps", 2, "-o", tmp_path)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "args.txt").read_text().split()[1:] == ["-n", "4096", "-iters", "5", "-steps", "2", "-o", str(tmp_path)]
    names = sorted(os.listdir(tmp_path))
    assert names == ["args.txt", "out0_0.000500.bin", "out2_0.000500.bin", "out4_0.000500.bin"], names
    for f in names[1:]:
        assert os.path.getsize(tmp_path / f) == 131072
    A, om, xi, om0 = F.kv_params()
    want = _engine_run(init2d(n, "kv", A, om), n, 5, xi, om0)
    got = np.fromfile(tmp_path / "out4_0.000500.bin", dtype=np.float64)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_input_file_and_gaussian(nbco, tmp_path):
    from coulomb_oscillators_amd import init2d
    n = 3000
    A, om, xi, om0 = F.kv_params()
    st = init2d(n, "kv", A, om)
    src = tmp_path / "in.bin"
    st.tofile(src)
    out = tmp_path / "o1"
    out.mkdir()
    r = run(nbco, "-iters", 1, "-steps", 1, "-xi", "%.17g" % xi, "-o", out, src)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out / "out1_0.000500.bin", dtype=np.float64)
    assert got.size == 4 * n and np.array_equal(got, _engine_run(st, n, 2, xi, om0))
    out2 = tmp_path / "o2"
    out2.mkdir()
    r = run(nbco, "-ga", "-n", 2048, "-iters", 0, "-o", out2)
    assert r.returncode == 0, r.stderr
    g = np.fromfile(out2 / "out0_0.000500.bin", dtype=np.float64)
    assert g.size == 4 * 2048 and np.isfinite(g).all()


@pytest.mark.gpu
def test_test_mode(nbco):
    r = run(nbco, "-test", "-n", 4096)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert any(l.startswith("Time elapsed: ") and l.endswith(" [s]") for l in lines)
    errs = [float(l.split(": Relative error: ")[1]) for l in lines if ": Relative error: " in l]
    assert len(errs) == 10 and all(np.isfinite(errs)) and errs[-1] < errs[0]
