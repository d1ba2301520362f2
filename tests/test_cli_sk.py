"""`nbco3 -sk <hx> <hy> <hz> <kx> <ky> <kz>` and `nbco -sk <hx> <hy> <kx> <ky>` on the GPU (coulomb_oscillators_amd/host): the snapshots are
byte-identical to a run without the flag; every sk<iter>_<ds>.bin is within TWICE the derived bound of `nbco3 -cpu -sk` on that very
snapshot (each is within the bound of the exact sums) and within the bound of the model of tests/sk_numpy.py; sk.txt names n_used and
the largest |rho_k|^2 / n_used of the file; with -aperture n_used follows n_left."""
import os
import subprocess

import numpy as np
import pytest

import sk_numpy as SK

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = (0, 2, 4)
H, KSTEP = (3, 2, 4), (700.0, 450.0, 900.0)


@pytest.fixture(scope="module")
def hosts(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return dict(nbco3=os.path.join(HOST, "nbco3"), nbco=os.path.join(HOST, "nbco"))


def run_ok(exe, folder, *args):
    folder.mkdir()
    r = subprocess.run([exe, *[str(a) for a in args], "-o", str(folder)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return folder


def rho_of(path, h):
    raw = np.fromfile(path, dtype=np.float64)
    assert raw.size == 2 * SK.count(h)
    return raw[0::2] + 1j * raw[1::2]


def check_line(ln, it, rho, used, h):
    """`iter n_used S_max ix iy [iz]` from the file's own rho, ties to the lowest index"""
    dim = len(h)
    ny, nz = 2 * h[1] + 1, (2 * h[2] + 1 if dim == 3 else 1)
    k0 = SK.index(h, 0, 0, 0)
    S = (rho.real ** 2 + rho.imag ** 2) / used
    S[k0] = -1.0
    at = int(np.argmax(S))
    assert len(ln) == 3 + dim and int(ln[0]) == it and int(ln[1]) == used and float(ln[2]) == S[at]
    assert [int(v) for v in ln[3:]] == [at // (ny * nz), at // nz % ny - h[1]] + ([at % nz - h[2]] if dim == 3 else [])


@pytest.mark.parametrize("extra,loses", [([], False), (["-aperture", "ellipsoid", 0.0075, 0.0025, 0.025, "-bath", 5.0, 5.0, 5.0, 1e-6, 1e-6, 1e-6, "-B", 0.0, 0.0, 3.0], True)])
def test_nbco3_gpu_files_agree_with_the_host_twin_and_the_model(hosts, tmp_path, extra, loses):
    n = 4096
    common = ["-n", n, "-p", 4, "-iters", 4, "-steps", 2, *extra]
    plain, logged = run_ok(hosts["nbco3"], tmp_path / "plain", *common), run_ok(hosts["nbco3"], tmp_path / "logged", *common, "-sk", *H, *KSTEP)
    assert not [f for f in os.listdir(plain) if f.startswith("sk")]
    lines = [ln.split() for ln in (logged / "sk.txt").read_text().splitlines()]
    assert len(lines) == len(ITERS)
    left = {it: n for it in ITERS}
    if loses:
        left = {int(ln.split()[0]): int(ln.split()[2]) for ln in (logged / "losses.txt").read_text().splitlines()}
        assert 0 < left[4] <= left[0] < n
    for k, it in enumerate(ITERS):
        name = "out%d_0.000500.bin" % it
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
        m = left[it]
        pos = np.fromfile(logged / name, dtype=np.float32)[:3 * m].reshape(m, 3)
        rho = rho_of(logged / ("sk%d_0.000500.bin" % it), H)
        re, im, used = SK.structure_factor(pos, H, KSTEP)
        err, lim = SK.error(rho, re, im), SK.bound(m, H)
        assert used == m and rho[SK.index(H, 0, 0, 0)] == complex(m, 0.0) and err <= lim
        check_line(lines[k], it, rho, m, H)
        # the host twin on this very snapshot: the program steps once before its first snapshot, and a step of 1e-30 moves no fp32 position
        twin = run_ok(hosts["nbco3"], tmp_path / ("twin%d" % it), "-cpu", "-cpu-threads", 4, "-iters", 0, "-ds", 1e-30, "-sk", *H, *KSTEP, logged / name)
        assert (twin / "out0_0.000000.bin").read_bytes()[:12 * m] == (logged / name).read_bytes()[:12 * m]
        host = rho_of(twin / "sk0_0.000000.bin", H)
        diff = np.abs(rho - host).max()
        print("iter %d n %d: device - model %.3g, device - host %.3g, bound %.3g" % (it, m, err, diff, lim))
        assert diff <= 2 * lim
        assert (twin / "sk.txt").read_text().split()[1] == str(m)


@pytest.mark.parametrize("n", [129, 3000])
def test_nbco_gpu_files_agree_with_the_model(hosts, tmp_path, n):
    h, kstep = (5, 3), (4000.0, 2500.0)
    common = ["-n", n, "-iters", 4, "-steps", 2]
    plain, logged = run_ok(hosts["nbco"], tmp_path / "plain", *common), run_ok(hosts["nbco"], tmp_path / "logged", *common, "-sk", *h, *kstep)
    assert not [f for f in os.listdir(plain) if f.startswith("sk")]
    lines = [ln.split() for ln in (logged / "sk.txt").read_text().splitlines()]
    assert len(lines) == len(ITERS)
    for k, it in enumerate(ITERS):
        name = "out%d_0.000500.bin" % it
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
        pos = np.fromfile(logged / name, dtype=np.float64)[:2 * n].reshape(n, 2)
        rho = rho_of(logged / ("sk%d_0.000500.bin" % it), h)
        re, im, used = SK.structure_factor(pos, h, kstep)
        err, lim = SK.error(rho, re, im), SK.bound(n, h)
        print("iter %d n %d: device - model %.3g, bound %.3g" % (it, n, err, lim))
        assert used == n and rho[SK.index(h, 0, 0)] == complex(n, 0.0) and err <= lim
        check_line(lines[k], it, rho, n, h)
