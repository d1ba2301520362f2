"""`nbco3 -corr` on the GPU: with `-snapshot-order input` the written out<iter>_*.bin files are the frames (row = particle number), so
corr.bin must match the long double model of tests/corr_numpy.py built from them; and `nbco3_dist -corr` is refused."""
import os
import subprocess

import numpy as np
import pytest

import corr_numpy as CN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
HALF = (0.0075, 0.0025, 0.025)         # 2.5 rms radii of the reference Gaussian
GPU = ["-n", 4096, "-p", 4, "-iters", 13, "-steps", 2, "-snapshot-order", "input"]
ITERS = (0, 2, 4, 6, 8, 10, 12)
DS = "0.000500"


@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_ok(exe, folder, *args):
    folder.mkdir()
    r = run(exe, *args, "-o", folder)
    assert r.returncode == 0, r.stderr
    return folder


def frames_of(folder, iters, n0, stride, aperture):
    """the trajectory buffer of the run from its snapshots in input order: rows are particle numbers; after a loss the rows of the
    file are the survivors in increasing number, and the loss files name who left"""
    rows = (n0 + stride - 1) // stride
    traj = np.full((rows, len(iters), 6), np.nan, dtype=np.float32)
    alive = np.ones(n0, dtype=bool)
    for it in ITERS:
        if aperture:
            raw = (folder / ("lost%d_%s.bin" % (it, DS))).read_bytes()
            alive[np.frombuffer(raw, dtype=np.int32, count=len(raw) // 28)] = False
        if it in iters:
            s = np.fromfile(folder / ("out%d_%s.bin" % (it, DS)), dtype=np.float32).reshape(2, -1, 3)
            ids = np.nonzero(alive)[0]
            assert s.shape[1] == len(ids)
            traj[:, iters.index(it)] = CN.scatter(np.concatenate([s[0].reshape(-1), s[1].reshape(-1)]), len(ids), ids, rows, stride)
    return traj


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "aperture", "bath"])
def test_corr_bin_is_the_model_of_the_snapshots(nbco3, tmp_path, variant):
    """six frames from iteration 2 on, every third particle, five lags"""
    extra = {"plain": [], "aperture": ["-aperture", "ellipsoid", *HALF], "bath": ["-bath", 2, 2, 2, 1e-6, 1e-6, 1e-6, "-B", 0, 0, 3]}[variant]
    out = run_ok(nbco3, tmp_path / "run", *GPU, "-corr", 3, 6, 5, "-corr-start", 1, *extra)
    traj = frames_of(out, ITERS[1:], 4096, 3, variant == "aperture")
    m = CN.model(traj, 6, 5)
    got = CN.records(np.fromfile(out / "corr.bin", dtype=np.uint8))
    print("nbco3 -corr, %s: worst fraction of the bound %.3g" % (variant, CN.check(got, m, variant)))
    rows = (4096 + 2) // 3
    if variant == "aperture":
        assert 0 < m["pairs"][0] < 6 * rows and np.isnan(traj).any()
    else:
        assert list(m["pairs"]) == [rows * k for k in (6, 5, 4, 3, 2)]
    from coulomb_oscillators_amd import time_corr_derive
    d = time_corr_derive(got)
    lines = [line.split() for line in (out / "corr.txt").read_text().splitlines()]
    assert len(lines) == 5
    for lag, words in enumerate(lines):
        assert int(words[0]) == lag and int(words[2]) == int(got["pairs"][lag]) and [float(w) for w in words[3:]] == list(d[lag])
        assert float(words[1]) == lag * (2 * float(np.float32(5e-4)))
    # the snapshots are those of the run without the flag
    plain = run_ok(nbco3, tmp_path / "plain", *GPU, *extra)
    for it in ITERS:
        assert (plain / ("out%d_%s.bin" % (it, DS))).read_bytes() == (out / ("out%d_%s.bin" % (it, DS))).read_bytes()


@pytest.mark.gpu
def test_tree_order_snapshots_record_the_same_frames(nbco3, tmp_path):
    """without `-snapshot-order input` the files are in tree order, the frames are not: corr.bin is the same bytes"""
    a = run_ok(nbco3, tmp_path / "input", *GPU, "-corr", 1, 7, 7)
    b = run_ok(nbco3, tmp_path / "tree", *GPU[:-2], "-corr", 1, 7, 7)
    assert (a / "corr.bin").read_bytes() == (b / "corr.bin").read_bytes() and os.path.getsize(a / "corr.bin") == 7 * 64


@pytest.mark.gpu
def test_nbco3_dist_refuses_the_flag(nbco3):
    r = run(os.path.join(HOST, "nbco3_dist"), "-n", 4096, "-corr", 1, 4, 4)
    assert r.returncode != 0 and "-corr" in r.stderr and "nbco3" in r.stderr
