"""`nbco3 -pairs <bins> <rmax>` (coulomb_oscillators_amd/host): at every snapshot <out>/pairs<iter>_<ds>.bin holds bins + 1 unsigned
64-bit counts and then n doubles of nn2 in the snapshot's particle order -- with `-cpu` from the pair rule on the host
(host/nbco_cpu.hpp), on the GPU from nbco_pair_hist_tree -- and the trajectory does not notice.  The rule has no tolerance: files
are compared integer for integer and bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import pairstat_numpy as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = (0, 2, 4)
SNAPS = ["out%d_0.000500.bin" % i for i in ITERS]
PAIRS = ["pairs%d_0.000500.bin" % i for i in ITERS]


@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_pair(exe, tmp_path, bins, rmax, *args):
    """the same run without and with -pairs; returns the folder of the second after checking that the snapshots are byte-identical"""
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-pairs", bins, rmax])):
        folder.mkdir()
        r = run(exe, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.startswith("out") and f.endswith(".bin")) == SNAPS
    assert not [f for f in os.listdir(plain) if f.startswith("pairs")]
    assert sorted(f for f in os.listdir(logged) if f.startswith("pairs")) == PAIRS
    for name in SNAPS:
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
    assert "-pairs" in (logged / "args.txt").read_text().split()
    return logged


def read_pairs(path, n, bins):
    raw = path.read_bytes()
    assert len(raw) == 8 * (bins + 1) + 8 * n
    return np.frombuffer(raw, dtype=np.uint64, count=bins + 1).astype(np.int64), np.frombuffer(raw, dtype=np.float64, offset=8 * (bins + 1))


def test_help_names_the_flag(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0 and "-pairs <bins> <rmax>" in r.stdout and "pairs<iter>_<ds>.bin" in r.stdout


def test_cpu_files_are_the_pair_statistics_of_the_snapshots(nbco3, tmp_path):
    n, bins, rmax = 512, 64, 0.002
    logged = run_pair(nbco3, tmp_path, bins, rmax, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    for snap, name in zip(SNAPS, PAIRS):
        pos = np.fromfile(logged / snap, dtype=np.float32).reshape(2, n, 3)[0]
        counts, nn2 = read_pairs(logged / name, n, bins)
        want = PN.pair_hist(pos, bins, rmax)
        assert 0 < want[0][:bins].sum() < want[0].sum() and np.isfinite(want[1]).any()
        assert np.array_equal(counts, want[0]), name
        assert nn2.tobytes() == want[1].tobytes(), name


def test_pairs_flag_is_refused_with_the_modes_that_do_not_simulate(nbco3, tmp_path):
    """as -moments: `-cpu -test` needs the GPU, and nothing is written; bad arguments are refused"""
    r = run(nbco3, "-cpu", "-test", "-pairs", 64, 0.002, "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("pairs")]
    for bad in ((0, 0.002), (64, 0), (70000, 0.002), (64, "nan")):
        r = run(nbco3, "-cpu", "-n", 16, "-pairs", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-pairs" in r.stderr, bad
    r = run(nbco3, "-cpu", "-n", 16, "-pairs", 64)
    assert r.returncode != 0


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["leapfrog", "pefrl"])
def test_gpu_files_are_pair_hist_of_the_snapshots(nbco3, tmp_path, integ):
    """`nbco3 -n 4096 -p 4 -iters 4 -steps 2 -pairs 64 0.002`: every file equals Engine.pair_hist (the exact form) of its snapshot,
    snapshots byte-identical to a run without the flag; also with PEFRL, which ends its step on a drift"""
    import torch
    from coulomb_oscillators_amd import Engine
    n, bins, rmax = 4096, 64, 0.002
    args = ["-n", n, "-p", 4, "-iters", 4, "-steps", 2] + ([] if integ == "leapfrog" else ["-integ", integ])
    logged = run_pair(nbco3, tmp_path, bins, rmax, *args)
    eng = Engine()
    try:
        for snap, name in zip(SNAPS, PAIRS):
            d = torch.from_numpy(np.fromfile(logged / snap, dtype=np.float32)).cuda()
            nn2 = torch.zeros(n, dtype=torch.float64, device="cuda")
            want = eng.pair_hist(d, n, bins, rmax, nn2=nn2).cpu().numpy()
            counts, got_nn2 = read_pairs(logged / name, n, bins)
            assert 0 < want[:bins].sum() < want.sum()
            assert np.array_equal(counts, want), name
            assert got_nn2.tobytes() == nn2.cpu().numpy().tobytes(), name
    finally:
        eng.close()
