"""The host side of the time correlations, no GPU: nbco_time_corr_derive, and `nbco3 -cpu -corr` against the long double model of
tests/corr_numpy.py built from the snapshots the same run wrote (with -cpu a snapshot row is a particle number until an aperture
loses somebody; then the numbers follow from the loss files)."""
import os
import subprocess

import numpy as np
import pytest

import corr_numpy as CN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
HALF = (0.0075, 0.0025, 0.025)         # 2.5 rms radii of the reference Gaussian


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


# ---- nbco_time_corr_derive --------------------------------------------------------------------------------------------------------
def test_derive_divides_the_sums(engine_lib):
    from coulomb_oscillators_amd import time_corr_derive, CORR_LAG
    assert np.dtype(CORR_LAG).itemsize == 64
    rec = np.zeros(4, dtype=CN.LAG)
    rec[0] = ((0.0, 0.0, 0.0), 0.0, (6.0, 3.0, 1.5), 3)                      # lag 0: msd = 0 gives alpha2 = 0, the vacf stays
    rec[1] = ((2.0, 4.0, 6.0), 50.0, (-1.0, 0.5, 0.25), 4)
    rec[2] = ((1.0, 2.0, 3.0), 7.0, (1.0, 1.0, 1.0), 0)                      # no pairs: zeros whatever the sums hold
    rec[3] = ((3.0, 3.0, 3.0), 5.0 / 3.0 * 9.0 * 9.0 / 1.0, (0.0, 0.0, 0.0), 1)
    out = time_corr_derive(rec)
    assert out.shape == (4, 8) and np.isfinite(out).all()
    assert np.array_equal(out[0], [0, 0, 0, 0, 0, 2.0, 1.0, 0.5])
    assert np.array_equal(out[1, :4], [0.5, 1.0, 1.5, 3.0]) and np.array_equal(out[1, 5:], [-0.25, 0.125, 0.0625])
    assert out[1, 4] == 3.0 * 12.5 / (5.0 * 9.0) - 1.0
    assert not out[2].any()
    assert out[3, 3] == 9.0 and abs(out[3, 4]) < 1e-15                       # <r^4> = 5/3 <r^2>^2: Gaussian displacements
    # a float64 view of the records is taken as well, and no lags at all is no work
    assert np.array_equal(time_corr_derive(rec.view(np.float64).reshape(4, 8)), out)
    assert time_corr_derive(rec[:0]).shape == (0, 8)


def test_derive_refuses_null_pointers(engine_lib):
    import ctypes as C
    from coulomb_oscillators_amd.engine import _load
    lib = _load()
    rec, out = np.zeros(1, dtype=CN.LAG), np.zeros(8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.nbco_time_corr_derive(None, 1, P(out)) == 2 and lib.nbco_time_corr_derive(P(rec), 1, None) == 2
    assert lib.nbco_time_corr_derive(P(rec), -1, P(out)) == 2 and lib.nbco_time_corr_derive(P(rec), 1, P(out)) == 0


# ---- nbco3 -cpu -corr -------------------------------------------------------------------------------------------------------------
CPU = ["-cpu", "-cpu-threads", 3, "-n", 512, "-ds", 0.05, "-iters", 61, "-steps", 10]
ITERS = (0, 10, 20, 30, 40, 50, 60)
DS = "0.050000"


def snap(folder, it):
    a = np.fromfile(folder / ("out%d_%s.bin" % (it, DS)), dtype=np.float32)
    return a.reshape(2, -1, 3)


def frames_of(folder, iters, n0, stride, aperture):
    """the trajectory buffer the run recorded, rebuilt from its snapshots: float32 [rows, len(iters), 6]"""
    rows = (n0 + stride - 1) // stride
    traj = np.full((rows, len(iters), 6), np.nan, dtype=np.float32)
    ids = np.arange(n0)
    for it in ITERS:
        if aperture:
            raw = (folder / ("lost%d_%s.bin" % (it, DS))).read_bytes()
            k = len(raw) // 28
            gone = np.zeros(len(ids), dtype=bool)
            gone[np.frombuffer(raw, dtype=np.int32, count=k)] = True
            ids = ids[~gone]
        if it in iters:
            s = snap(folder, it)
            assert s.shape[1] == len(ids)
            state = np.concatenate([s[0].reshape(-1), s[1].reshape(-1)])
            traj[:, iters.index(it)] = CN.scatter(state, len(ids), ids, rows, stride)
    return traj


def read_txt(folder):
    return [line.split() for line in (folder / "corr.txt").read_text().splitlines()]


@pytest.mark.parametrize("aperture", [False, True])
def test_cpu_files_follow_the_model_of_the_snapshots(nbco3, tmp_path, aperture):
    """frames at the iterations 10 .. 50 (-corr-start 5, five frames), every second particle, four lags"""
    extra = ["-aperture", "ellipsoid", *HALF] if aperture else []
    out = run_ok(nbco3, tmp_path / "run", *CPU, "-corr", 2, 5, 4, "-corr-start", 5, *extra)
    iters = ITERS[1:6]
    traj = frames_of(out, iters, 512, 2, aperture)
    m = CN.model(traj, 5, 4)
    got = CN.records(np.fromfile(out / "corr.bin", dtype=np.uint8))
    print("nbco3 -cpu -corr, aperture %s: worst fraction of the bound %.3g" % (aperture, CN.check(got, m, "cpu")))
    if aperture:
        assert 0 < m["pairs"][0] < 5 * 256 and np.isnan(traj).any()
    else:
        assert list(m["pairs"]) == [256 * 5, 256 * 4, 256 * 3, 256 * 2]
    # corr.txt: lag, tau = lag * steps * ds, pairs, and nbco_time_corr_derive of the records
    from coulomb_oscillators_amd import time_corr_derive
    d = time_corr_derive(got)
    lines = read_txt(out)
    assert len(lines) == 4
    for lag, words in enumerate(lines):
        assert len(words) == 11 and int(words[0]) == lag and int(words[2]) == int(got["pairs"][lag])
        assert float(words[1]) == lag * (10 * float(np.float32(0.05)))
        assert [float(w) for w in words[3:]] == list(d[lag])
    # the run itself does not notice
    plain = run_ok(nbco3, tmp_path / "plain", *CPU, *extra)
    for it in ITERS:
        assert (plain / ("out%d_%s.bin" % (it, DS))).read_bytes() == (out / ("out%d_%s.bin" % (it, DS))).read_bytes()


def test_a_short_run_writes_the_lags_its_frames_allow(nbco3, tmp_path):
    """a window of 50 frames, 20 lags, and a run that ends after seven snapshots: seven lags"""
    out = run_ok(nbco3, tmp_path / "run", *CPU, "-corr", 1, 50, 20)
    got = CN.records(np.fromfile(out / "corr.bin", dtype=np.uint8))
    traj = frames_of(out, ITERS, 512, 1, False)
    CN.check(got, CN.model(traj, 7, 7), "short")
    assert len(read_txt(out)) == 7
    none = run_ok(nbco3, tmp_path / "none", *CPU, "-corr", 1, 50, 20, "-corr-start", 1000)
    assert (none / "corr.bin").read_bytes() == b"" and (none / "corr.txt").read_text() == ""


def test_flag_refusals_and_help(nbco3, tmp_path):
    for bad in ((0, 4, 4), (1, 4, 5), (1, 4, 0), (1, 2049, 4), (1, "x", 4)):
        r = run(nbco3, "-cpu", "-n", 16, "-corr", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-corr" in r.stderr, bad
    assert run(nbco3, "-cpu", "-n", 16, "-corr", 1, 4).returncode != 0
    r = run(nbco3, "-cpu", "-n", 16, "-corr", 1, 4, 4, "-corr-start", -1, "-o", tmp_path)
    assert r.returncode != 0 and "-corr-start" in r.stderr
    for mode in (["-test"], ["-test2"], ["-accuracy", 0.01]):
        r = run(nbco3, "-n", 64, *mode, "-corr", 1, 4, 4, "-o", tmp_path)
        assert r.returncode != 0 and "-corr" in r.stderr, mode
    assert not [f for f in os.listdir(tmp_path) if f.startswith("corr")]
    r = run(nbco3, "-h")
    assert r.returncode == 0
    for text in ("-corr <stride> <frames> <lags>", "-corr-start <iter>", "corr.bin", "corr.txt", "fused pass"):
        assert text in r.stdout, text
