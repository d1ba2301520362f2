"""`nbco3 -moments` and `nbco -moments` (coulomb_oscillators_amd/host): <out>/moments.txt gets a `#` line naming the columns and at
every snapshot `iter`, the means, then per plane `sig_q sig_p cov_qp emit halo_q halo` -- with `nbco3 -cpu` from the two-pass fp64
sums on the host (host/nbco_cpu.hpp), on the GPU from nbco_beam_moments / nbco_2d_beam_moments -- and the trajectory does not notice."""
import os
import subprocess

import numpy as np
import pytest

import beam_numpy as BN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
SNAPS = ["out0_0.000500.bin", "out2_0.000500.bin", "out4_0.000500.bin"]


@pytest.fixture(scope="module")
def hosts(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return dict(nbco3=os.path.join(HOST, "nbco3"), nbco=os.path.join(HOST, "nbco"))


def run(exe, *args):
    return subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)


def run_pair(exe, tmp_path, *args):
    """the same run without and with -moments; returns the folder of the second after checking that the snapshots are byte-identical"""
    plain, logged = tmp_path / "plain", tmp_path / "logged"
    for folder, extra in ((plain, []), (logged, ["-moments"])):
        folder.mkdir()
        r = run(exe, *args, *extra, "-o", folder)
        assert r.returncode == 0, r.stderr
        assert sorted(f for f in os.listdir(folder) if f.endswith(".bin")) == SNAPS
    assert not (plain / "moments.txt").exists()
    for name in SNAPS:
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
    assert "-moments" in (logged / "args.txt").read_text().split()
    return logged


def rows_of(folder, dim):
    """the three rows of moments.txt after checking the header line, the column count and the number format"""
    cols = 1 + 2 * dim + 6 * dim
    lines = (folder / "moments.txt").read_text().splitlines()
    assert len(lines) == 4 and lines[0].startswith("# iter mean_x ")
    names = lines[0][1:].split()
    assert len(names) == cols and len(set(names)) == cols
    assert names[1 + 2 * dim:7 + 2 * dim] == ["sig_x", "sig_vx", "cov_x_vx", "emit_x", "halo_q_x", "halo_x"]
    rows = np.loadtxt(folder / "moments.txt", ndmin=2)
    assert rows.shape == (3, cols) and rows[:, 0].tolist() == [0, 2, 4]
    for line in lines[1:]:
        t = line.split()
        assert t[0] in ("0", "2", "4") and all("%.17g" % float(v) == v for v in t[1:])          # %.17g
    return rows


def row_of(m, dim):
    """columns 1.. of a row, from a Moments structure or the reference's dict"""
    get = (lambda k: np.array(m[k])) if isinstance(m, dict) else (lambda k: np.array(getattr(m, k)))
    cov = get("cov")
    out = list(get("mean")[:2 * dim])
    for k in range(dim):
        out += [np.sqrt(cov[k, k]), np.sqrt(cov[dim + k, dim + k]), cov[k, dim + k], get("emit")[k], get("halo_q")[k], get("halo")[k]]
    return np.array(out)


def test_help_names_the_flag(hosts):
    for exe in hosts.values():
        r = run(exe, "-h")
        assert r.returncode == 0 and "-moments" in r.stdout and "moments.txt" in r.stdout


def test_cpu_rows_are_the_moments_of_the_snapshots(hosts, tmp_path):
    """`nbco3 -cpu -moments -n 512 -iters 4 -steps 2`: three rows.  Means, variances (sig^2) and cov_qp are sums: each within
    1e-10 x (mean absolute value of its terms) of the reference on the snapshot file's state -- the bound of the GPU test, a
    sequential fp64 sum of 512 terms errs by far less.  emit, halo_q and halo are functions of those sums; for this beam (plane
    correlation below 0.2, so I2 is no cancellation) a handful of 1e-10 relative errors add up to less than 1e-8 x (value + 2)."""
    n = 512
    logged = run_pair(hosts["nbco3"], tmp_path, "-cpu", "-cpu-threads", 3, "-n", n, "-iters", 4, "-steps", 2)
    rows = rows_of(logged, 3)
    for row, name in zip(rows, SNAPS):
        ref = BN.moments(np.fromfile(logged / name, dtype=np.float32), 3)
        sc = ref["scale"]
        assert (np.abs(row[1:7] - ref["mean"]) <= 1e-10 * sc["mean"]).all(), (name, "mean")
        for k in range(3):
            sq, sp, cqp, emit, halo_q, halo = row[7 + 6 * k:13 + 6 * k]
            r = abs(ref["cov"][k, 3 + k]) / np.sqrt(ref["cov"][k, k] * ref["cov"][3 + k, 3 + k])
            assert r < 0.2
            assert abs(sq * sq - ref["cov"][k, k]) <= 1e-10 * sc["cov"][k, k], (name, k, "sig_q")
            assert abs(sp * sp - ref["cov"][3 + k, 3 + k]) <= 1e-10 * sc["cov"][3 + k, 3 + k], (name, k, "sig_p")
            assert abs(cqp - ref["cov"][k, 3 + k]) <= 1e-10 * sc["cov"][k, 3 + k], (name, k, "cov_qp")
            assert abs(emit - ref["emit"][k]) <= 1e-8 * ref["emit"][k], (name, k, "emit")
            assert abs(halo_q - ref["halo_q"][k]) <= 1e-8 * (ref["halo_q"][k] + 2), (name, k, "halo_q")
            assert abs(halo - ref["halo"][k]) <= 1e-8 * (ref["halo"][k] + 2), (name, k, "halo")


def test_moments_flag_is_refused_with_the_modes_that_do_not_simulate(hosts, tmp_path):
    """as -energy: `-cpu -test` needs the GPU, and nothing is written"""
    r = run(hosts["nbco3"], "-cpu", "-test", "-moments", "-o", tmp_path)
    assert r.returncode != 0 and "need the GPU" in r.stderr
    assert not (tmp_path / "moments.txt").exists()


def _close(got, want):
    return (np.abs(got - want) <= 1e-12 * np.abs(want)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("integ", ["leapfrog", "pefrl"])
def test_gpu_rows_are_beam_moments_of_the_snapshots(hosts, tmp_path, integ):
    """`nbco3 -n 4096 -p 4 -iters 4 -steps 2 -moments`: rows equal Engine.beam_moments of the snapshot files within 1e-12, snapshots
    byte-identical to a run without the flag; also with PEFRL, which ends its step on a drift"""
    import torch
    from coulomb_oscillators_amd import Engine
    n = 4096
    args = ["-n", n, "-p", 4, "-iters", 4, "-steps", 2] + ([] if integ == "leapfrog" else ["-integ", integ])
    logged = run_pair(hosts["nbco3"], tmp_path, *args)
    rows = rows_of(logged, 3)
    eng = Engine()
    try:
        for row, name in zip(rows, SNAPS):
            d = torch.from_numpy(np.fromfile(logged / name, dtype=np.float32)).cuda()
            want = row_of(eng.beam_moments(d, n), 3)
            assert np.isfinite(want).all() and _close(row[1:], want), (name, row[1:], want)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 129])
def test_gpu_2d_rows_are_beam_moments_2d_of_the_snapshots(hosts, tmp_path, n):
    """`nbco -n N -iters 4 -steps 2 -moments` against Engine.beam_moments_2d of the snapshot files within 1e-12.  The program accepts
    any n >= 1; n = 2 is the smallest whose sampled state is finite (one particle, centred and rescaled to the requested rms, is
    0 / 0), and 129 is the smallest n the original program accepts."""
    import torch
    from coulomb_oscillators_amd import Engine
    logged = run_pair(hosts["nbco"], tmp_path, "-n", n, "-iters", 4, "-steps", 2)
    rows = rows_of(logged, 2)
    eng = Engine()
    try:
        for row, name in zip(rows, SNAPS):
            d = torch.from_numpy(np.fromfile(logged / name, dtype=np.float64)).cuda()
            want = row_of(eng.beam_moments_2d(d, n), 2)
            assert np.isfinite(want).all() and _close(row[1:], want), (name, row[1:], want)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_2d_moments_with_test_mode_has_no_effect(hosts, tmp_path):
    r = run(hosts["nbco"], "-test", "-moments", "-n", 1024, "-o", tmp_path)
    assert r.returncode == 0, r.stderr
    assert os.listdir(tmp_path) == []
