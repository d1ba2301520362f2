"""`nbco3 -modes <hx> <hy> <hz> <kx> <ky> <kz> <frames> <lags>` (coulomb_oscillators_amd/host), with -cpu and, in one GPU case, on the
device: the sizes of modes.bin, modes_derived.bin and modes.txt; modes.bin against the long double model of tests/modes_numpy.py fed
from the snapshots the same run wrote -- the program correlates its own records, each within the derived bounds of the exact ones
(rho: sk_numpy.bound; j_c: modes_numpy.j_bound), so the sums are held to the model within the rounding bounds plus what those record
errors can move them by (modes_numpy.propagated); the derived file and the columns of modes.txt from the file's own records; the
snapshots byte-identical to a run without the flag; the refusals of nbco3 and of nbco3_dist."""
import os
import subprocess

import numpy as np
import pytest

import modes_numpy as MN
import sk_numpy as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
H, KSTEP = (2, 1, 2), (700.0, 450.0, 900.0)
K = SK.count(H)
LOSSY = ["-aperture", "ellipsoid", 0.0075, 0.0025, 0.025, "-bath", 5.0, 5.0, 5.0, 1e-6, 1e-6, 1e-6, "-B", 0.0, 0.0, 3.0]


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


def check_files(out, plain, n, iters, frames, lags):
    """the three files of a run whose frames are the snapshots `iters`"""
    from coulomb_oscillators_amd import mode_corr_derive, MODE_LAG
    F, Lg = len(iters), min(lags, len(iters))
    assert F <= frames
    got = np.fromfile(out / "modes.bin", dtype=MODE_LAG)
    assert os.path.getsize(out / "modes.bin") == K * Lg * 64 and os.path.getsize(out / "modes_derived.bin") == K * Lg * 32
    got = got.reshape(K, Lg)
    left = {it: n for it in iters}
    if (out / "losses.txt").exists():
        left = {int(ln.split()[0]): int(ln.split()[2]) for ln in (out / "losses.txt").read_text().splitlines()}
    series, E8, used_all = np.zeros((K, F, 8), dtype=MN.L), np.zeros(8), []
    for f, it in enumerate(iters):
        name = "out%d_0.000500.bin" % it
        if plain is not None:
            assert (plain / name).read_bytes() == (out / name).read_bytes(), name
        m = left[it]
        snap = np.fromfile(out / name, dtype=np.float32)
        assert snap.size == 6 * m
        rec, used, V = MN.records(snap[:3 * m].reshape(m, 3), snap[3 * m:].reshape(m, 3), H, KSTEP)
        assert used == m
        series[:, f, :] = rec
        used_all.append(used)
        jb = MN.j_bound(m, H, V)
        E8 = np.maximum(E8, [SK.bound(m, H)] * 2 + [jb[0]] * 2 + [jb[1]] * 2 + [jb[2]] * 2)
    lag_list = list(range(Lg))
    worst = MN.held_with_records(got, MN.correlate(series, H, KSTEP, F, lag_list=lag_list), MN.propagated(series, E8, H, KSTEP, F, lag_list))
    print("modes.bin against the model of the snapshots: worst fraction of the bound %.3g" % worst)
    assert worst <= 1.0
    # s0 at lag 0 and k = 0 is the exact sum of the exact counts
    k0 = SK.index(H, 0, 0, 0)
    assert got["s0"][k0, 0, 0] == sum(used_all) and got["s0"][k0, 0, 1] == 0.0
    n_norm = sum(used_all) / F
    d = mode_corr_derive(got, H, KSTEP, n_norm)
    assert np.fromfile(out / "modes_derived.bin", dtype=np.float64).tobytes() == d.tobytes()
    lines = [ln.split() for ln in (out / "modes.txt").read_text().splitlines()]
    kv = MN.wave_vectors(H, KSTEP)
    idx = MN.wave_vectors(H, (1.0, 1.0, 1.0))
    assert len(lines) == K
    for k, ln in enumerate(lines):
        assert len(ln) == 8 and [int(q) for q in ln[:3]] == [int(q) for q in idx[k]]
        assert float(ln[3]) == np.sqrt(kv[k, 0] * kv[k, 0] + kv[k, 1] * kv[k, 1] + kv[k, 2] * kv[k, 2])
        assert [float(q) for q in ln[4:]] == d[k, 0].tolist()
    assert d[k0, 0, 0] > 0.9 * n_norm          # F(0, 0) = <N^2> / <N>


@pytest.mark.parametrize("variant", ["plain", "lossy"])
def test_cpu_files_are_the_model_of_the_snapshots(nbco3, tmp_path, variant):
    n = 300
    extra = LOSSY if variant == "lossy" else []
    common = ["-cpu", "-cpu-threads", 4, "-n", n, "-iters", 8, "-steps", 2, *extra]
    plain = run_ok(nbco3, tmp_path / "plain", *common)
    assert not [f for f in os.listdir(plain) if f.startswith("modes")]
    out = run_ok(nbco3, tmp_path / "run", *common, "-modes", *H, *KSTEP, 4, 3, "-modes-start", 2)
    check_files(out, plain, n, (2, 4, 6, 8), 4, 3)


def test_cpu_run_that_ends_early_writes_what_it_has(nbco3, tmp_path):
    n = 200
    out = run_ok(nbco3, tmp_path / "short", "-cpu", "-cpu-threads", 4, "-n", n, "-iters", 4, "-steps", 2, "-modes", *H, *KSTEP, 100, 50)
    check_files(out, None, n, (0, 2, 4), 100, 50)
    none = run_ok(nbco3, tmp_path / "none", "-cpu", "-cpu-threads", 4, "-n", n, "-iters", 2, "-steps", 2, "-modes", *H, *KSTEP, 4, 2, "-modes-start", 50)
    assert [os.path.getsize(none / f) for f in ("modes.bin", "modes_derived.bin", "modes.txt")] == [0, 0, 0]


def test_refusals(nbco3):
    good = [*H, *KSTEP, 4, 3]
    bad = [[*H, *KSTEP, 4], [65, 1, 2, *KSTEP, 4, 3], [-1, 1, 2, *KSTEP, 4, 3], [*H, 0.0, 450.0, 900.0, 4, 3], [*H, 700.0, "nan", 900.0, 4, 3],
           [*H, *KSTEP, 4, 5], [*H, *KSTEP, 4, 0], [*H, *KSTEP, 1025, 3], [*H, *KSTEP, "x", 3], [*H, *KSTEP, 4, "3.5"]]
    for args in bad:
        r = run(nbco3, "-cpu", "-n", 100, "-modes", *args)
        assert r.returncode != 0 and "-modes" in r.stderr, args
    for start in (-1, "x"):
        r = run(nbco3, "-cpu", "-n", 100, "-modes", *good, "-modes-start", start)
        assert r.returncode != 0 and "-modes-start" in r.stderr
    for mode in (["-test"], ["-test2"], ["-accuracy", 0.01]):
        r = run(nbco3, "-n", 100, "-modes", *good, *mode)
        assert r.returncode != 0 and "-modes" in r.stderr and "cannot be combined" in r.stderr, mode


def test_nbco3_dist_refuses_the_flag(nbco3):
    for flag, args in (("-modes", [*H, *KSTEP, 4, 3]), ("-modes-start", [2])):
        r = run(os.path.join(HOST, "nbco3_dist"), "-n", 4096, flag, *args)
        assert r.returncode != 0 and flag in r.stderr and "nbco3" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "lossy"])
def test_gpu_files_are_the_model_of_the_snapshots(nbco3, tmp_path, variant):
    n = 4096
    extra = LOSSY if variant == "lossy" else []
    common = ["-n", n, "-p", 4, "-iters", 8, "-steps", 2, *extra]
    plain = run_ok(nbco3, tmp_path / "plain", *common)
    out = run_ok(nbco3, tmp_path / "run", *common, "-modes", *H, *KSTEP, 4, 3, "-modes-start", 2)
    check_files(out, plain, n, (2, 4, 6, 8), 4, 3)
