"""`nbco3 -slices` and `nbco -slices` (coulomb_oscillators_amd/host): at every snapshot <out>/slices<iter>_<ds>.txt gets a `#` line
naming the columns, a `# outside <k>` line and per slice `s lo_s n`, the means, then per plane `sig_q sig_p cov_qp emit halo_q halo`
-- with `nbco3 -cpu` from the bin rule and the two-pass fp64 sums on the host (host/nbco_cpu.hpp), on the GPU from
nbco_slice_moments / nbco_2d_slice_moments -- and the trajectory does not notice."""
import os
import subprocess

import numpy as np
import pytest

import slice_numpy as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ITERS = [0, 2, 4]
COORD = {"x": 0, "y": 1, "z": 2, "vx": 3, "vy": 4, "vz": 5}


@pytest.fixture(scope="module")
def hosts(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return dict(nbco3=os.path.join(HOST, "nbco3"), nbco=os.path.join(HOST, "nbco"))


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_pair(exe, tmp_path, flag, *args):
    """the same run without and with -slices; returns the folder of the second after checking that the snapshots are byte-identical"""
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-slices", *flag])):
        folder.mkdir()
        r = run(exe, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
    snaps = ["out%d_0.000500.bin" % i for i in ITERS]
    assert sorted(f for f in os.listdir(plain) if f != "args.txt") == snaps
    assert sorted(f for f in os.listdir(logged) if f != "args.txt") == snaps + ["slices%d_0.000500.txt" % i for i in ITERS]
    for name in snaps:
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
    return logged


def table_of(path, dim, flag):
    """(tokens of the rows, n_outside) of a slice file after checking the two `#` lines, the column count, s, lo_s and the format"""
    bins, lo, hi = int(flag[1]), float(flag[2]), float(flag[3])
    cols = 3 + 2 * dim + 6 * dim
    lines = path.read_text().splitlines()
    assert len(lines) == 2 + bins and lines[0].startswith("# s lo_s n mean_x ")
    names = lines[0][1:].split()
    assert len(names) == cols and len(set(names)) == cols
    assert names[3 + 2 * dim:9 + 2 * dim] == ["sig_x", "sig_vx", "cov_x_vx", "emit_x", "halo_q_x", "halo_x"]
    head = lines[1].split()
    assert head[:2] == ["#", "outside"] and len(head) == 3
    rows = [line.split() for line in lines[2:]]
    for s, t in enumerate(rows):
        assert len(t) == cols and t[0] == str(s) and t[2] == str(int(t[2]))
        assert abs(float(t[1]) - (lo + s * (hi - lo) / bins)) <= 1e-15 * max(abs(lo), abs(hi))   # (a few roundings at the size of the edges)
        assert all("%.17g" % float(v) == v for v in t[1:2] + t[3:])          # %.17g
    return rows, int(head[2])


def test_help_names_the_flag(hosts):
    for exe in hosts.values():
        r = run(exe, "-h")
        assert r.returncode == 0 and "-slices" in r.stdout and "slices<iter>_<ds>.txt" in r.stdout


def test_cpu_rows_are_the_slices_of_the_snapshots(hosts, tmp_path):
    """`nbco3 -cpu -slices z 8 -0.013 0.017 -n 512 -iters 4 -steps 2`: one file per snapshot.  Counts and the `outside` line equal the
    reference on the snapshot file's state; means, variances (sig^2) and cov_qp are sums: each within 1e-10 x (mean absolute value of
    its terms within the slice) of the reference -- the bound of the GPU test; a sequential fp64 sum of at most 512 terms errs by
    far less.  emit, halo_q and halo are functions of the slice's sums and are held to the reference's within what that bound on
    every sum allows to first order, doubled for the higher orders (derived_bounds): a slice's I2 and I4 may be cancellations, so
    the bounds carry the slice's own condition instead of one figure for all."""
    n, flag = 512, ["z", 8, -0.013, 0.017]
    logged = run_pair(hosts["nbco3"], tmp_path, flag, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    assert "-slices" in (logged / "args.txt").read_text().split()
    for i in ITERS:
        rows, outside = table_of(logged / ("slices%d_0.000500.txt" % i), 3, flag)
        st = np.fromfile(logged / ("out%d_0.000500.bin" % i), dtype=np.float32)
        ref, ref_outside = SN.slice_moments(st, 3, (COORD["z"], *flag[1:]))
        assert outside == ref_outside and 0 < outside < n
        for t, r in zip(rows, ref):
            assert int(t[2]) == r["n"] > 2
            row, sc = np.array([float(v) for v in t]), r["scale"]
            assert (np.abs(row[3:9] - r["mean"]) <= 1e-10 * sc["mean"]).all(), (i, t[0], "mean")
            for k in range(3):
                sq, sp, cqp, emit, halo_q, halo = row[9 + 6 * k:15 + 6 * k]
                assert abs(sq * sq - r["cov"][k, k]) <= 1e-10 * sc["cov"][k, k], (i, t[0], k, "sig_q")
                assert abs(sp * sp - r["cov"][3 + k, 3 + k]) <= 1e-10 * sc["cov"][3 + k, 3 + k], (i, t[0], k, "sig_p")
                assert abs(cqp - r["cov"][k, 3 + k]) <= 1e-10 * sc["cov"][k, 3 + k], (i, t[0], k, "cov_qp")
                tol = derived_bounds(r, 3, k)
                assert r["emit"][k] > 0 and r["halo"][k] > -2 and max(tol) < 1e-6     # (no plane of these slices is degenerate)
                assert abs(emit - r["emit"][k]) <= tol[0], (i, t[0], k, "emit", emit, r["emit"][k])
                assert abs(halo_q - r["halo_q"][k]) <= tol[1], (i, t[0], k, "halo_q", halo_q, r["halo_q"][k])
                assert abs(halo - r["halo"][k]) <= tol[2], (i, t[0], k, "halo", halo, r["halo"][k])


def derived_bounds(r, dim, k, eps=1e-10):
    """what an error of eps x (mean absolute term) in every sum of the reference record r allows in (emit, halo_q, halo) of plane k:
    I2 = x2 e2 - xe^2, emit = sqrt(I2), halo_q + 2 = f0 / x2^2, I4 = f0 f4 + 3 f2^2 - 4 f3 f1, halo + 2 = sqrt(3 I4) / (2 I2);
    first-order propagation with every term taken absolute, times 2"""
    cov, m4, sc, sm = r["cov"], r["m4"][k], r["scale"]["cov"], r["scale"]["m4"][k]
    x2, e2, xe = cov[k, k], cov[dim + k, dim + k], cov[k, dim + k]
    dx2, de2, dxe = eps * sc[k, k], eps * sc[dim + k, dim + k], eps * sc[k, dim + k]
    df = eps * sm
    i2 = x2 * e2 - xe * xe
    i4 = m4[0] * m4[4] + 3 * m4[2] ** 2 - 4 * m4[3] * m4[1]
    di2 = dx2 * e2 + x2 * de2 + 2 * abs(xe) * dxe
    di4 = df[0] * m4[4] + m4[0] * df[4] + 6 * abs(m4[2]) * df[2] + 4 * abs(m4[3]) * df[1] + 4 * abs(m4[1]) * df[3]
    assert i2 > 0 and i4 > 0
    return (2 * di2 / (2 * np.sqrt(i2)), 2 * (df[0] / x2 ** 2 + 2 * m4[0] * dx2 / x2 ** 3),
            2 * (np.sqrt(3 * i4) / (2 * i2)) * (di4 / (2 * i4) + di2 / i2))


def test_slices_flag_refuses_bad_arguments_before_anything_is_written(hosts, tmp_path):
    for exe, dim in ((hosts["nbco3"], 3), (hosts["nbco"], 2)):
        for bad in (["w", 8, -1, 1], ["z" if dim == 2 else "r", 8, -1, 1], ["x", 0, -1, 1], ["x", 65537, -1, 1], ["x", "8abc", -1, 1], ["x", "1e3", -1, 1],
                    ["x", "99999999999999999999", -1, 1], ["x", "", -1, 1], ["x", 8, 1, 1], ["x", 8, 2, 1],
                    ["x", 8, "nan", 1], ["x", 8, -1, "inf"], ["x", 8, -1], ["x"]):
            r = run(exe, "-n", 64, "-o", tmp_path, "-slices", *bad)
            assert r.returncode != 0 and "'-slices'" in r.stderr, (exe, bad, r.stderr)
            assert ("missing" if len(bad) < 4 else "invalid") in r.stderr, (exe, bad, r.stderr)
            assert os.listdir(tmp_path) == [], (exe, bad)


def test_slices_flag_is_refused_with_the_modes_that_do_not_simulate(hosts, tmp_path):
    """as -moments: `-cpu -test` needs the GPU, and nothing is written"""
    r = run(hosts["nbco3"], "-cpu", "-test", "-slices", "z", 8, -0.013, 0.017, "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert os.listdir(tmp_path) == []


def check_gpu_rows(logged, dim, n, flag, fn, dtype):
    import torch
    for i in ITERS:
        rows, outside = table_of(logged / ("slices%d_0.000500.txt" % i), dim, flag)
        d = torch.from_numpy(np.fromfile(logged / ("out%d_0.000500.bin" % i), dtype=dtype)).cuda()
        recs, want_outside = fn(d, n, (COORD[flag[0]], *flag[1:]))
        assert outside == want_outside and 0 < outside < n
        for t, m in zip(rows, recs):
            cov = np.array(m.cov)
            want = [m.n] + list(np.array(m.mean)[:2 * dim])
            for k in range(dim):
                want += [np.sqrt(cov[k, k]), np.sqrt(cov[dim + k, dim + k]), cov[k, dim + k], m.emit[k], m.halo_q[k], m.halo[k]]
            assert t[2] == str(m.n) and t[3:] == ["%.17g" % v for v in want[1:]], (i, t[0])
        assert sum(m.n for m in recs) + outside == n and max(m.n for m in recs) > 2


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["leapfrog", "pefrl"])
def test_gpu_rows_are_slice_moments_of_the_snapshots(hosts, tmp_path, integ):
    """`nbco3 -n 4096 -p 4 -iters 4 -steps 2 -slices vz 12 ..`: the rows equal Engine.slice_moments of the snapshot files to the 17
    digits printed, snapshots byte-identical to a run without the flag; also with PEFRL, which ends its step on a drift"""
    from coulomb_oscillators_amd import Engine
    n, flag = 4096, ["vz", 12, -0.011, 0.016]
    args = ["-n", n, "-p", 4, "-iters", 4, "-steps", 2] + ([] if integ == "leapfrog" else ["-integ", integ])
    logged = run_pair(hosts["nbco3"], tmp_path, flag, *args)
    eng = Engine()
    try:
        check_gpu_rows(logged, 3, n, flag, eng.slice_moments, np.float32)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [129, 3000])
def test_gpu_2d_rows_are_slice_moments_2d_of_the_snapshots(hosts, tmp_path, n):
    """`nbco -n N -iters 4 -steps 2 -slices x 8 -0.001 0.0015` against Engine.slice_moments_2d of the snapshot files"""
    from coulomb_oscillators_amd import Engine
    flag = ["x", 8, -0.001, 0.0015]
    logged = run_pair(hosts["nbco"], tmp_path, flag, "-n", n, "-iters", 4, "-steps", 2)
    eng = Engine()
    try:
        check_gpu_rows(logged, 2, n, flag, eng.slice_moments_2d, np.float64)
    finally:
        eng.close()
