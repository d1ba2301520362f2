"""`nbco3 -probes points.bin` (coulomb_oscillators_amd/host/nbco3.cpp): at every snapshot <out>/probes<iter>_<ds>.bin gets m x 3 doubles
of field and m doubles of potential at the points of the file -- with -cpu the exact fp64 sums on the host, on the GPU from
nbco_probe_tree -- and the trajectory does not notice."""
import os
import subprocess

import numpy as np
import pytest

import probe3d_numpy as p3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
SNAPS = ["out0_0.000500.bin", "out2_0.000500.bin", "out4_0.000500.bin"]
PROBES = ["probes0_0.000500.bin", "probes2_0.000500.bin", "probes4_0.000500.bin"]


@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def points(oracle32, n, tmp_path):
    """a probe file for the n-particle reference ball: points in 1.5 x its box, some of them on particles"""
    pos = oracle32.init_reference(n)[0]
    t = p3.probe_sets(pos, 9)["box1.5"][:300]
    t[::10] = pos[:30]
    path = tmp_path / "points.bin"
    t.astype(np.float32).tofile(path)
    return t, path


def run_pair(nbco3, tmp_path, pts, *args):
    """the same run without and with -probes; returns the two output folders after checking that the snapshots are byte-identical"""
    plain, probed = tmp_path / "plain", tmp_path / "probed"
    for folder, extra in ((plain, []), (probed, ["-probes", pts])):
        folder.mkdir()
        r = run(nbco3, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.startswith("out")) == SNAPS
    assert not [f for f in os.listdir(plain) if f.startswith("probes")]
    assert sorted(f for f in os.listdir(probed) if f.startswith("probes")) == PROBES
    for name in SNAPS:
        assert (plain / name).read_bytes() == (probed / name).read_bytes(), name
    return plain, probed


def test_cpu_probe_files_are_the_exact_sums_of_the_snapshots(nbco3, oracle32, tmp_path):
    """`nbco3 -cpu -probes -n 512 -iters 4 -steps 2`: three files, field and potential within 1e-12 of the largest sum of |terms| of
    the fp64 sums over the snapshot's positions (both fp64 over the same fp32 values: only the arithmetic's rounding differs)"""
    n = 512
    t, path = points(oracle32, n, tmp_path)
    m = len(t)
    _, probed = run_pair(nbco3, tmp_path, path, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    par0 = float(oracle32.params(n)[0])
    for snap, name in zip(SNAPS, PROBES):
        pos = np.fromfile(probed / snap, dtype=np.float32).reshape(2, n, 3)[0]
        out = np.fromfile(probed / name, dtype=np.float64)
        assert out.shape == (4 * m,)
        a, psi = out[:3 * m].reshape(m, 3), out[3 * m:]
        ea, epsi, mag = p3.exact(pos, t, 1e-18, with_abs=True)
        assert np.abs(a - par0 * ea).max() <= 1e-12 * par0 * mag.max(), name
        assert np.abs(psi - par0 * epsi).max() <= 1e-12 * par0 * epsi.max(), name


def test_bad_probe_files_are_refused(nbco3, tmp_path):
    (tmp_path / "odd.bin").write_bytes(b"\0" * 40)                # not a multiple of 12
    (tmp_path / "empty.bin").write_bytes(b"")
    for name, word in (("odd.bin", "multiple of 12"), ("empty.bin", "empty"), ("missing.bin", "cannot read")):
        r = run(nbco3, "-cpu", "-n", 64, "-iters", 0, "-probes", tmp_path / name, "-o", tmp_path)
        assert r.returncode != 0 and word in r.stderr, (name, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("probes") or f.startswith("out")]
    r = run(nbco3, "-probes")
    assert r.returncode != 0 and "missing argument" in r.stderr


def test_nbco3_dist_refuses_the_flag(nbco3, tmp_path):
    (tmp_path / "p.bin").write_bytes(b"\0" * 12)
    r = run(os.path.join(HOST, "nbco3_dist"), "-gpus", 2, "-n", 8192, "-probes", tmp_path / "p.bin", "-o", tmp_path)
    assert r.returncode != 0 and "'-probes' is not available with kd-domain sharding" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["leapfrog", "pefrl"])
def test_gpu_probe_files_are_probe_tree_of_the_snapshots(nbco3, oracle32, tmp_path, integ):
    """`nbco3 -n 4096 -p 4 -iters 4 -steps 2 -probes`: the files equal Engine.probe_tree on the snapshot files at the same options
    bit for bit, snapshots byte-identical to a run without the flag; also with PEFRL, which ends its step on a drift"""
    import torch
    from coulomb_oscillators_amd import Engine
    n, p = 4096, 4
    t, path = points(oracle32, n, tmp_path)
    m = len(t)
    args = ["-n", n, "-p", p, "-iters", 4, "-steps", 2] + ([] if integ == "leapfrog" else ["-integ", integ])
    _, probed = run_pair(nbco3, tmp_path, path, *args)
    prm = torch.from_numpy(oracle32.params(n)).cuda()
    td = torch.from_numpy(t).cuda()
    eng = Engine(fmm_order=p, tree_steps=8, m2l_first=1)          # the program's options (host/nbco3.cpp)
    try:
        for snap, name in zip(SNAPS, PROBES):
            d = torch.from_numpy(np.fromfile(probed / snap, dtype=np.float32)).cuda()
            out = torch.full((4 * m,), float("nan"), dtype=torch.float64, device="cuda")
            eng.probe_tree(d, n, td, m, prm, out[:3 * m], out[3 * m:])
            got = np.fromfile(probed / name, dtype=np.float64)
            assert np.array_equal(got, out.cpu().numpy()), name
    finally:
        eng.close()
