"""Bond-orientational order without a GPU: nbco_bond_harmonics against the addition theorem, the numpy model of tests/bond_numpy.py
against the closed forms of the ideal lattices, and `nbco3 -cpu -bonds` (the host twin of host/nbco_cpu.hpp, which takes its harmonics
from the header the device kernels use) against the model.  Squares are compared with the tolerance derived for nb <= 256
(bond_numpy.TOL2); counts compare as integers."""
import math
import os
import subprocess

import numpy as np
import pytest

import bond_numpy as BN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = (0, 2, 4)
SNAPS = ["out%d_0.000500.bin" % i for i in ITERS]
BONDS = ["bonds%d_0.000500.bin" % i for i in ITERS]


def test_harmonics_obey_the_addition_theorem(engine_lib):
    """sum_m Y_lm(u) Y_lm(v) = (2l + 1) / (4 pi) P_l(u . v) for 200 random pairs of unit vectors: a wrong constant or sign shows here"""
    from coulomb_oscillators_amd import bond_harmonics
    rng = np.random.default_rng(2024)
    for _ in range(200):
        u, v = rng.normal(size=3), rng.normal(size=3)
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        (a4, a6), (b4, b6) = bond_harmonics(u), bond_harmonics(v)
        assert a4.shape == (9,) and a6.shape == (13,)
        t = float(u @ v)
        assert abs(a4 @ b4 - 9.0 / (4.0 * math.pi) * BN.legendre(4, t)) < 1e-13
        assert abs(a6 @ b6 - 13.0 / (4.0 * math.pi) * BN.legendre(6, t)) < 1e-13
        assert max(np.abs(a4).max(), np.abs(a6).max()) <= 1.02


def test_harmonics_at_the_pole_and_bad_arguments(engine_lib):
    import ctypes as C
    from coulomb_oscillators_amd import bond_harmonics, EngineError
    y4, y6 = bond_harmonics([0.0, 0.0, 1.0])
    assert abs(y4[0] - math.sqrt(9.0 / (4.0 * math.pi))) < 1e-15 and abs(y6[0] - math.sqrt(13.0 / (4.0 * math.pi))) < 1e-15
    assert not y4[1:].any() and not y6[1:].any()
    with pytest.raises(EngineError):
        bond_harmonics([float("nan"), 0.0, 1.0])
    L = C.CDLL(engine_lib)
    buf = (C.c_double * 13)()
    assert L.nbco_bond_harmonics(None, buf, buf) == 2 and L.nbco_bond_harmonics(buf, None, buf) == 2 and L.nbco_bond_harmonics(buf, buf, None) == 2


@pytest.mark.parametrize("name,rmax2,nb,q4,q6", BN.IDEAL)
def test_model_gives_the_closed_forms_of_the_ideal_lattices(name, rmax2, nb, q4, q6):
    """the central particle of the sc, bcc and fcc lattices (integer fp32 coordinates); the sc cutoff is
    rmax^2 = 1.5, under which nb = 6 and q4 = sqrt(7 / 12) hold (rmax = 1.5 would take in the 12 second neighbours)"""
    pos, centre = BN.LATTICES[name]()
    m = BN.bond_order(pos, math.sqrt(rmax2))
    assert m["nb"][centre] == nb and m["nb_max"] == nb
    assert abs(math.sqrt(m["q2"][centre, 0]) - q4) < 1e-7 and abs(math.sqrt(m["q2"][centre, 1]) - q6) < 1e-7


def test_model_in_two_dimensions():
    pos, centre = BN.square2d()
    m = BN.bond_order(pos, 1.2)
    assert m["nb"][centre] == 4 and abs(m["q2"][centre, 0] - 1.0) < BN.TOL2 and abs(m["q2"][centre, 1]) < BN.TOL2
    pos, centre = BN.triangular2d()
    m = BN.bond_order(pos, 1.2)
    assert m["nb"][centre] == 6 and abs(m["q2"][centre, 1] - 1.0) < BN.TOL2 and abs(m["q2"][centre, 0]) < BN.TOL2


def test_model_global_q_by_moments_is_the_legendre_double_sum():
    """the moment form of the global Q_l^2 against the plain double sum over all bonds, on a cloud and on a lattice; and the rule's
    edges: coincident particles are not neighbours, a NaN is outside"""
    rng = np.random.default_rng(5)
    pos = rng.normal(size=(300, 3)).astype(np.float32)
    m = BN.bond_order(pos, 0.6)
    assert 0 < m["isolated"] < 300 and m["nb_max"] <= 256
    for k, l in enumerate((4, 6)):
        assert abs(m["Q2"][k] - BN.global_q2_double_sum(pos, 0.6, l)) < 1e-13
    lat, _ = BN.fcc(2)
    m = BN.bond_order(lat, math.sqrt(3.0))
    for k, l in enumerate((4, 6)):
        assert abs(m["Q2"][k] - BN.global_q2_double_sum(lat, math.sqrt(3.0), l)) < 1e-13
    pos[7] = pos[3]
    pos[11, 1] = np.nan
    m = BN.bond_order(pos, 0.6)
    i, d, _ = BN.bonds(pos, 0.6)
    assert m["nb"][11] == 0 and not (i == 11).any() and np.isfinite(d).all() and np.isfinite(m["q2"]).all()
    assert m["nb"][3] == m["nb"][7] and np.array_equal(m["q2"][3], m["q2"][7])


# ---- nbco3 -cpu -bonds ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_pair(exe, tmp_path, rmax, *args):
    """the same run without and with -bonds; returns the folder of the second after checking that the snapshots are byte-identical"""
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-bonds", rmax])):
        folder.mkdir()
        r = run(exe, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.startswith("out") and f.endswith(".bin")) == SNAPS
    assert not [f for f in os.listdir(plain) if f.startswith("bonds")]
    assert sorted(f for f in os.listdir(logged) if f.startswith("bonds")) == sorted(BONDS + ["bonds.txt"])
    for name in SNAPS:
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
    assert "-bonds" in (logged / "args.txt").read_text().split()
    return logged


def read_bonds(path, n):
    raw = path.read_bytes()
    assert len(raw) == 4 * n + 16 * n
    return np.frombuffer(raw, dtype=np.int32, count=n).astype(np.int64), np.frombuffer(raw, dtype=np.float64, offset=4 * n).reshape(n, 2)


def check_against_model(folder, n, rmax):
    """every bonds file and every line of bonds.txt against the model of its snapshot"""
    lines = [ln.split() for ln in (folder / "bonds.txt").read_text().splitlines()]
    assert [int(ln[0]) for ln in lines] == list(ITERS) and all(len(ln) == 8 for ln in lines)
    for snap, name, ln in zip(SNAPS, BONDS, lines):
        pos = np.fromfile(folder / snap, dtype=np.float32).reshape(2, n, 3)[0]
        nb, q = read_bonds(folder / name, n)
        m = BN.bond_order(pos, rmax)
        assert 0 < m["isolated"] < n and 2 <= m["nb_max"] <= 256   # (the run exercises both the nb = 0 path and real sums)
        assert np.array_equal(nb, m["nb"]), name
        assert np.isfinite(q).all() and not q[nb == 0].any()
        assert np.abs(q * q - m["q2"]).max() < BN.TOL2, name
        assert [int(ln[1]), int(ln[2]), int(ln[3])] == [m["bonds"], m["isolated"], m["nb_max"]]
        q_mean, Q = np.array([float(ln[4]), float(ln[5])]), np.array([float(ln[6]), float(ln[7])])
        assert np.abs(q_mean - m["q_mean"]).max() < BN.TOL_MEAN
        assert np.abs(Q * Q - m["Q2"]).max() < BN.TOL2


def test_help_names_the_flag(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0 and "-bonds <rmax>" in r.stdout and "bonds<iter>_<ds>.bin" in r.stdout and "bonds.txt" in r.stdout


def test_cpu_files_are_the_bond_order_of_the_snapshots(nbco3, tmp_path):
    n, rmax = 512, 0.0012
    logged = run_pair(nbco3, tmp_path, rmax, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    check_against_model(logged, n, rmax)


def test_bonds_flag_is_refused_where_pairs_is(nbco3, tmp_path):
    """`-cpu -test` needs the GPU, and nothing is written; bad arguments are refused"""
    r = run(nbco3, "-cpu", "-test", "-bonds", 0.002, "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("bonds")]
    for bad in (0, -1, "nan", "inf"):
        r = run(nbco3, "-cpu", "-n", 16, "-bonds", bad, "-o", tmp_path)
        assert r.returncode != 0 and "-bonds" in r.stderr, bad
    r = run(nbco3, "-cpu", "-n", 16, "-bonds")
    assert r.returncode != 0
