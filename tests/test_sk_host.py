"""The static structure factor without a GPU: nbco_sk_phase (the one phase rule of csrc/structure_factor.hpp, exported host-only) against
long double, and `nbco3 -cpu -sk` (the host twin of host/nbco_cpu.hpp, which forms its phases and products from the same header)
against the model of tests/sk_numpy.py within the derived bound n u (8 (hx + hy + hz + 1) + n).  (`nbco -sk`, the 2-D program, has no
host evaluator: tests/test_cli_sk.py holds it to the model on the GPU.)"""
import os
import subprocess

import numpy as np
import pytest

import sk_numpy as SK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = (0, 2, 4)
SNAPS = ["out%d_0.000500.bin" % i for i in ITERS]
H, KSTEP = (3, 2, 4), (700.0, 450.0, 900.0)


# ---- nbco_sk_phase -----------------------------------------------------------------------------------------------------------------------
def test_phase_is_within_four_units_of_long_double(engine_lib):
    from coulomb_oscillators_amd import sk_phase
    t = np.random.default_rng(7).uniform(-50.0, 50.0, 200000)
    got = np.array([sk_phase(v) for v in t])
    r = (t - np.rint(t)).astype(SK.L)            # exact in fp64
    ang = SK.TWO_PI * r
    ec, es = np.abs(got[:, 0] - np.cos(ang)).max(), np.abs(got[:, 1] - np.sin(ang)).max()
    print("phase: cos %.3f u, sin %.3f u" % (float(ec / SK.U), float(es / SK.U)))
    assert ec <= 4 * SK.U and es <= 4 * SK.U
    # the same over the reduced interval itself, dense near the quarter turns where the quadrants meet
    t = np.concatenate([np.linspace(-0.5, 0.5, 20001), 0.125 + np.linspace(-1e-9, 1e-9, 2001), -0.375 + np.linspace(-1e-9, 1e-9, 2001)])
    got = np.array([sk_phase(v) for v in t])
    ang = SK.TWO_PI * (t - np.rint(t)).astype(SK.L)
    assert np.abs(got[:, 0] - np.cos(ang)).max() <= 4 * SK.U and np.abs(got[:, 1] - np.sin(ang)).max() <= 4 * SK.U


def test_phase_exact_values_symmetry_and_bad_arguments(engine_lib):
    import ctypes as C
    from coulomb_oscillators_amd import sk_phase, EngineError
    from coulomb_oscillators_amd.engine import _load
    for t in (0.0, 1.0, -3.0, 17.0, 2.0 ** 40, 2.0 ** 60, -2.0 ** 53):
        assert sk_phase(t) == (1.0, 0.0), t
    for t in (0.25, 1.25, -2.75, 1000.25):
        assert sk_phase(t) == (0.0, 1.0), t
    for t in (0.5, -0.5, 1.5, -7.5, 1000.5):
        assert sk_phase(t) == (-1.0, 0.0), t
    for t in (0.75, -0.25, 5.75):
        assert sk_phase(t) == (0.0, -1.0), t
    for t in np.random.default_rng(8).uniform(-50.0, 50.0, 2000).tolist() + [0.125, 0.375, 0.1, 1e-300, 49.999999]:
        c, s = sk_phase(t)
        assert sk_phase(-t) == (c, -s), t
        assert abs(c * c + s * s - 1.0) <= 16 * SK.U
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(EngineError):
            sk_phase(bad)
    assert _load().nbco_sk_phase(0.5, None) == 2   # NBCO_ERR_ARG


# ---- nbco3 -cpu -sk ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def read_rho(path, h):
    raw = np.fromfile(path, dtype=np.float64)
    assert raw.size == 2 * SK.count(h)
    return raw[0::2] + 1j * raw[1::2]


def check_folder(folder, n, h, kstep, factor=1.0, n_of=None):
    """every sk file and every line of sk.txt against the model of its snapshot"""
    lines = [ln.split() for ln in (folder / "sk.txt").read_text().splitlines()]
    assert [int(ln[0]) for ln in lines] == list(ITERS) and all(len(ln) == 6 for ln in lines)
    ny, nz = 2 * h[1] + 1, 2 * h[2] + 1
    for snap, ln in zip(SNAPS, lines):
        raw = np.fromfile(folder / snap, dtype=np.float32)
        m = raw.size // 6 if n_of is None else n_of[snap]
        pos = raw[:3 * m].reshape(m, 3)
        rho = read_rho(folder / snap.replace("out", "sk"), h)
        re, im, used = SK.structure_factor(pos, h, kstep)
        err, lim = SK.error(rho, re, im), SK.bound(m, h)
        print("%s: n %d error %.3g, bound %.3g" % (snap, m, err, lim))
        assert err <= factor * lim
        k0 = SK.index(h, 0, 0, 0)
        assert rho[k0] == complex(used, 0.0) and int(ln[1]) == used == m
        # S_max and its place, from the file's own rho: ties to the lowest index
        S = (rho.real ** 2 + rho.imag ** 2) / used
        S[k0] = -1.0
        at = int(np.argmax(S))
        assert float(ln[2]) == S[at] and S[at] > 1.0
        assert [int(v) for v in ln[3:]] == [at // (ny * nz), at // nz % ny - h[1], at % nz - h[2]]


def test_help_names_the_flag(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0 and "-sk <hx> <hy> <hz> <kx> <ky> <kz>" in r.stdout and "sk<iter>_<ds>.bin" in r.stdout and "sk.txt" in r.stdout


def test_cpu_files_are_the_structure_factor_of_the_snapshots(nbco3, tmp_path):
    """the same run without and with -sk: byte-identical snapshots, the files against the model; a rerun with another number of threads
    writes the same bytes"""
    n = 512
    common = ["-cpu", "-n", n, "-iters", 4, "-steps", 2]
    folders = {}
    for name, extra in (("plain", ["-cpu-threads", 3]), ("logged", ["-cpu-threads", 3, "-sk", *H, *KSTEP]), ("again", ["-cpu-threads", 5, "-sk", *H, *KSTEP])):
        folders[name] = tmp_path / name
        folders[name].mkdir()
        r = run(nbco3, *common, *extra, "-o", folders[name])
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folders[name]) if f.startswith("out") and f.endswith(".bin")) == SNAPS
    plain, logged, again = folders["plain"], folders["logged"], folders["again"]
    assert not [f for f in os.listdir(plain) if f.startswith("sk")]
    names = sorted([s.replace("out", "sk") for s in SNAPS] + ["sk.txt"])
    assert sorted(f for f in os.listdir(logged) if f.startswith("sk")) == names
    for s in SNAPS:
        assert (plain / s).read_bytes() == (logged / s).read_bytes(), s
    for f in names:
        assert (logged / f).read_bytes() == (again / f).read_bytes(), f
    assert "-sk" in (logged / "args.txt").read_text().split()
    check_folder(logged, n, H, KSTEP)


def test_cpu_with_aperture_bath_and_field(nbco3, tmp_path):
    """-sk beside -aperture, -bath and -B: n_used follows n_left"""
    n = 512
    r = run(nbco3, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2, "-sk", *H, *KSTEP, "-aperture", "ellipsoid", 0.012, 0.012, 0.012,
            "-bath", 5.0, 5.0, 5.0, 1e-6, 1e-6, 1e-6, "-B", 0.0, 0.0, 3.0, "-o", tmp_path)
    assert r.returncode == 0, r.stderr
    left = {int(ln.split()[0]): int(ln.split()[2]) for ln in (tmp_path / "losses.txt").read_text().splitlines()}
    assert 0 < left[4] <= left[2] <= left[0] < n
    check_folder(tmp_path, n, H, KSTEP, n_of={s: left[i] for s, i in zip(SNAPS, ITERS)})


def test_sk_flag_refusals(nbco3, tmp_path):
    """`-cpu -test` needs the GPU, and nothing is written; bad arguments are refused; the sharded program refuses the flag"""
    r = run(nbco3, "-cpu", "-test", "-sk", *H, *KSTEP, "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("sk")]
    for bad in ([-1, 2, 2, 1, 1, 1], [2, 65, 2, 1, 1, 1], [2, 2, "x", 1, 1, 1], [2, 2, 2, 0, 1, 1], [2, 2, 2, 1, -1, 1], [2, 2, 2, 1, 1, "nan"],
                [2, 2, 2, 1, "inf", 1], [2.5, 2, 2, 1, 1, 1]):
        r = run(nbco3, "-cpu", "-n", 16, "-sk", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-sk" in r.stderr, bad
    r = run(nbco3, "-cpu", "-n", 16, "-sk", 2, 2, 2, 1, 1)
    assert r.returncode != 0
    r = run(os.path.join(HOST, "nbco3_dist"), "-sk", *H, *KSTEP)
    assert r.returncode != 0 and "'-sk' is not available" in r.stderr
    r = run(os.path.join(HOST, "nbco"), "-sk", 2, 65, 1, 1, "-o", tmp_path)
    assert r.returncode != 0 and "-sk" in r.stderr
