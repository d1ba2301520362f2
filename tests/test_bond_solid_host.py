"""Crystalline-particle detection without a GPU: nbco_bond_coherence against the numpy rule bit for bit, the numpy model of
tests/solid_numpy.py on the ideal lattices and on a random gas (the figures that say the measure discriminates), and `nbco3 -cpu -solid`
(the host twin of host/nbco_cpu.hpp, built from the header functions the device kernels use) against the model.  Integers compare as
integers, squares of q-bar with bond_numpy.TOL2."""
import math
import os
import subprocess

import numpy as np
import pytest

import bond_numpy as BN
import solid_numpy as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = (0, 2, 4)
SNAPS = ["out%d_0.000500.bin" % i for i in ITERS]
SOLID = ["solid%d_0.000500.bin" % i for i in ITERS]
DMIN = 0.7


# ---- the coherence ------------------------------------------------------------------------------------------------------------------------
def test_coherence_is_the_numpy_rule_bit_for_bit(engine_lib):
    """10^4 random record pairs: products, then adds from the left, each rounded once -- a contracted multiply-add differs in the last
    bit in most of them; the same bits from either end; NULL is refused"""
    import ctypes as C
    L = C.CDLL(engine_lib)
    L.nbco_bond_coherence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(77)
    e, f = rng.normal(size=(10000, SN.VEC)), rng.normal(size=(10000, SN.VEC))
    for v in (e, f):
        v[:, 9:22] /= np.linalg.norm(v[:, 9:22], axis=1)[:, None]
    want = SN.coherence(e, f)
    got, back = np.zeros(10000), np.zeros(10000)
    for k in range(10000):
        assert L.nbco_bond_coherence(e[k].ctypes.data, f[k].ctypes.data, got[k:].ctypes.data) == 0
        assert L.nbco_bond_coherence(f[k].ctypes.data, e[k].ctypes.data, back[k:].ctypes.data) == 0
    assert got.tobytes() == want.tobytes() and back.tobytes() == got.tobytes()
    exact = np.array([math.fsum(e[k, 9:22] * f[k, 9:22]) for k in range(100)])
    assert np.abs(got[:100] - exact).max() < 1.5e-15   # (and it is the dot product: 13 roundings of at most 2^-53 each)
    assert L.nbco_bond_coherence(None, f.ctypes.data, got.ctypes.data) == 2 and L.nbco_bond_coherence(e.ctypes.data, None, got.ctypes.data) == 2
    assert L.nbco_bond_coherence(e.ctypes.data, f.ctypes.data, None) == 2


def test_coherence_of_a_unit_vector_with_itself(engine_lib):
    from coulomb_oscillators_amd import bond_coherence, BOND_VEC
    assert BOND_VEC == SN.VEC
    rng = np.random.default_rng(78)
    for _ in range(100):
        v = rng.normal(size=BOND_VEC)
        v[9:22] /= np.linalg.norm(v[9:22])
        assert abs(bond_coherence(v, v) - 1.0) < 1e-15
        w = rng.normal(size=BOND_VEC)
        assert bond_coherence(v, w) == bond_coherence(w, v) == float(SN.coherence(v, w))   # entries outside [9, 22) do not enter
        w[:9], w[22:] = 0.0, 0.0
        assert bond_coherence(v, w) == float(SN.coherence(v, w))


# ---- the model discriminates -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rmax2,coord,full,aligned,floor", [("sc", 1.5, 6, 1331, 1331, 0.83), ("bcc", 3.5, 8, 686, 684, 0.62), ("fcc", 3.0, 12, 171, 171, 0.77)])
def test_model_on_the_ideal_lattices(engine_lib, name, rmax2, coord, full, aligned, floor):
    """bond_numpy's lattices at dmin = 0.7: the particles with the full coordination, those whose bonds are all solid, and the smallest
    d6 of any bond, surface included; the centre has xi = nb and a q-bar_6 equal to its q6 (every neighbour has its environment)"""
    pos, centre = BN.LATTICES[name]()
    m = SN.solid(pos, math.sqrt(rmax2), DMIN, coord)
    assert m["nb"].max() == coord and (m["nb"] == coord).sum() == full
    assert m["xi"].max() == m["xi_max"] == coord and (m["xi"] == coord).sum() == m["n_solid"] == aligned
    assert floor <= m["d6"].min() < floor + 0.01 and m["d6"].max() <= 1.0 + 1e-15
    assert m["solid_bonds"] % 2 == 0 and m["xi"][centre] == m["nb"][centre] == coord
    q6 = [row[4] for row in BN.IDEAL if row[0] == name and row[1] == rmax2][0]
    assert abs(math.sqrt(m["qbar2"][centre, 1]) - q6) < 1e-7


def test_model_on_a_random_gas(engine_lib):
    """1025 uniform points with 12 neighbours in the bulk sphere (9.9 on average, the surface included): 1.4 % of the bonds pass
    d6 > 0.7, no particle has more than 3 of them, and no d6 is closer to the threshold than 1e-3 -- far above the rounding of a record"""
    pos, rmax = SN.gas()
    assert len(pos) == 1025 and abs(rmax - 0.14086) < 1e-5
    m = SN.solid(pos, rmax, DMIN, 7)
    assert abs(m["nb"].mean() - 9.9) < 0.05
    assert abs((m["d6"] > DMIN).mean() - 0.014) < 0.001
    assert m["xi"].max() == m["xi_max"] == 3 and m["n_solid"] == 0 and m["solid_bonds"] % 2 == 0
    assert 0.9e-3 < np.abs(m["d6"] - DMIN).min() < 1.1e-3
    assert SN.solid(pos, rmax, -2.0, 0)["xi"].tolist() == m["nb"].tolist() and not SN.solid(pos, rmax, 2.0, 0)["xi"].any()


def test_model_records(engine_lib):
    """the records of the model: unit q^ where a_l > 0, zeros for an isolated particle, a_l q^_lm = S_lm / nb, q_l = sqrt(4 pi/(2l+1)) a_l"""
    pos = np.random.default_rng(5).normal(size=(300, 3)).astype(np.float32)
    nb, vec = SN.records(pos, 0.6)
    ref = BN.bond_order(pos, 0.6)
    assert np.array_equal(nb, ref["nb"]) and 0 < (nb == 0).sum() < 300
    assert not vec[nb == 0].any() and np.isfinite(vec).all()
    for lo, hi, a, Q in ((0, 9, 22, SN.Q4), (9, 22, 23, SN.Q6)):
        on = vec[:, a] > 0
        assert np.array_equal(on, nb > 0)
        assert np.abs((vec[on, lo:hi] ** 2).sum(axis=1) - 1.0).max() < 1e-14
        assert np.abs(Q * vec[:, a] ** 2 - ref["q2"][:, 0 if lo == 0 else 1]).max() < BN.TOL2


# ---- nbco3 -cpu -solid ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def read_solid(path, n):
    raw = path.read_bytes()
    assert len(raw) == 4 * n + 4 * n + 16 * n
    nb, xi = np.frombuffer(raw, dtype=np.int32, count=n).astype(np.int64), np.frombuffer(raw, dtype=np.int32, count=n, offset=4 * n).astype(np.int64)
    return nb, xi, np.frombuffer(raw, dtype=np.float64, offset=8 * n).reshape(n, 2)


def test_help_names_the_flag(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0 and "-solid <rmax> <dmin> <xi_min>" in r.stdout and "solid<iter>_<ds>.bin" in r.stdout and "solid.txt" in r.stdout


def test_cpu_files_are_the_solid_pass_of_the_snapshots(nbco3, tmp_path):
    """the same run without and with -solid: byte-identical snapshots; every solid file and every line of solid.txt against the model of its
    snapshot.  The twin's records differ from the model's by rounding (1e-13), so the test asserts first that no bond of the model
    is closer to dmin than 1e-9: xi is then the same integer."""
    n, rmax, dmin, xi_min = 512, 0.0012, 0.3, 2
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-solid", rmax, dmin, xi_min])):
        folder.mkdir()
        r = run(nbco3, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.startswith("out") and f.endswith(".bin")) == SNAPS
    assert not [f for f in os.listdir(plain) if f.startswith("solid")]
    assert sorted(f for f in os.listdir(logged) if f.startswith("solid")) == sorted(SOLID + ["solid.txt"])
    assert "-solid" in (logged / "args.txt").read_text().split()
    lines = [ln.split() for ln in (logged / "solid.txt").read_text().splitlines()]
    assert [int(ln[0]) for ln in lines] == list(ITERS) and all(len(ln) == 6 for ln in lines)
    for snap, name, ln in zip(SNAPS, SOLID, lines):
        assert (plain / snap).read_bytes() == (logged / snap).read_bytes(), snap
        pos = np.fromfile(logged / snap, dtype=np.float32).reshape(2, n, 3)[0]
        m = SN.solid(pos, rmax, dmin, xi_min)
        assert 0 < m["isolated"] < n and 2 <= m["nb"].max() <= 256 and 0 < m["n_solid"] < n - m["isolated"]   # (both outcomes of every branch)
        assert np.abs(m["d6"] - dmin).min() > 1e-9
        nb, xi, qbar = read_solid(logged / name, n)
        assert np.array_equal(nb, m["nb"]) and np.array_equal(xi, m["xi"]), name
        assert np.isfinite(qbar).all() and not qbar[nb == 0].any()
        assert np.abs(qbar * qbar - m["qbar2"]).max() < BN.TOL2, name
        assert [int(ln[1]), int(ln[2]), int(ln[3])] == [m["n_solid"], m["solid_bonds"], m["xi_max"]]
        assert np.abs(np.array([float(ln[4]), float(ln[5])]) - m["qbar_mean"]).max() < BN.TOL_MEAN


def test_solid_flag_is_refused_where_bonds_is(nbco3, tmp_path):
    """`-cpu -test` needs the GPU, and nothing is written; bad and missing arguments are refused"""
    r = run(nbco3, "-cpu", "-test", "-solid", 0.002, 0.7, 7, "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("solid")]
    for bad in ((0, 0.7, 7), (-1, 0.7, 7), ("nan", 0.7, 7), ("inf", 0.7, 7), (0.002, "nan", 7), (0.002, "inf", 7), (0.002, 0.7, -1), (0.002, 0.7, "x"),
                (0.002, 0.7, 1.5), (0.002, 0.7, 1 << 40)):
        r = run(nbco3, "-cpu", "-n", 16, "-solid", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-solid" in r.stderr, bad
    for short in ((), (0.002,), (0.002, 0.7)):
        r = run(nbco3, "-cpu", "-n", 16, "-solid", *short)
        assert r.returncode != 0 and "-solid" in r.stderr, short
