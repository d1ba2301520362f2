"""`nbco3 -energy` (coulomb_oscillators_amd/host/nbco3.cpp): <out>/energy.txt gets `iter kinetic elastic coulomb total` at every
snapshot -- with -cpu from the exact fp64 pair sum on the host (host/nbco_cpu.hpp), on the GPU from nbco_energy_tree -- and the
trajectory does not notice."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
EXE = os.path.join(HOST, "nbco3")
SNAPS = ["out0_0.000500.bin", "out2_0.000500.bin", "out4_0.000500.bin"]


@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_pair(nbco3, tmp_path, *args):
    """the same run without and with -energy; returns the two output folders after checking that the snapshots are byte-identical"""
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-energy"])):
        folder.mkdir()
        r = run(nbco3, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.endswith(".bin")) == SNAPS
    assert not (plain / "energy.txt").exists()
    for name in SNAPS:
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
    assert "-energy" in (logged / "args.txt").read_text().split()
    return plain, logged


def rows_of(folder):
    rows = np.loadtxt(folder / "energy.txt", ndmin=2)
    assert rows.shape == (3, 5) and rows[:, 0].tolist() == [0, 2, 4]
    for r in rows:
        assert r[4] == r[1] + r[2] + r[3]                       # total is the sum of its row
    text = (folder / "energy.txt").read_text().split()
    assert all("%.17g" % float(t) == t for t in text[1:5])                                 # %.17g
    return rows


def test_help_names_the_flag(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0 and "-energy" in r.stdout and "energy.txt" in r.stdout


def test_cpu_energy_rows_are_the_exact_energy_of_the_snapshots(nbco3, oracle32, oracle64, tmp_path):
    """`nbco3 -cpu -energy -n 512 -iters 4 -steps 2`: three rows, each within 1e-10 of oracle64.energy of the snapshot file's state
    (both fp64 over the same fp32 state: only the summation order differs)"""
    n = 512
    _, logged = run_pair(nbco3, tmp_path, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    rows = rows_of(logged)
    par = oracle32.params(n).astype(np.float64)
    for row, name in zip(rows, SNAPS):
        state = np.fromfile(logged / name, dtype=np.float32).reshape(2, n, 3).astype(np.float64)
        want = oracle64.energy(state, par, threads=4)
        assert np.abs(row[1:4] - want).max() <= 1e-10 * np.abs(want).max(), (name, row, want)
        assert abs(row[4] - want.sum()) <= 1e-10 * want.sum()


def test_energy_flag_is_ignored_by_the_modes_that_do_not_simulate(nbco3, tmp_path):
    r = run(nbco3, "-cpu", "-test", "-energy", "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not (tmp_path / "energy.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["leapfrog", "pefrl"])
def test_gpu_energy_rows_are_energy_tree_of_the_snapshots(nbco3, oracle32, tmp_path, integ):
    """`nbco3 -n 4096 -p 4 -iters 4 -steps 2 -energy`: rows equal Engine.energy_tree on the snapshot files at the same options within
    1e-12, snapshots byte-identical to a run without the flag; also with PEFRL, which ends its step on a drift"""
    import torch
    from coulomb_oscillators_amd import Engine
    n, p = 4096, 4
    args = ["-n", n, "-p", p, "-iters", 4, "-steps", 2] + ([] if integ == "leapfrog" else ["-integ", integ])
    _, logged = run_pair(nbco3, tmp_path, *args)
    rows = rows_of(logged)
    prm = torch.from_numpy(oracle32.params(n)).cuda()
    eng = Engine(fmm_order=p, tree_steps=8, m2l_first=1)          # the program's options (host/nbco3.cpp)
    try:
        for row, name in zip(rows, SNAPS):
            d = torch.from_numpy(np.fromfile(logged / name, dtype=np.float32)).cuda()
            want = eng.energy_tree(d, n, prm)
            assert np.abs(row[1:4] - want).max() <= 1e-12 * np.abs(want).max(), (name, row, want)
    finally:
        eng.close()
