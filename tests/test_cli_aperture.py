"""`nbco3 -aperture <ellipsoid|box> <hx> <hy> <hz>` / `nbco -aperture <ellipse|box> <hx> <hy>` (coulomb_oscillators_amd/host): at every
snapshot iteration the particles outside leave the run -- with `-cpu` by the rule on the host (host/nbco_cpu.hpp), on the GPU through
nbco_aperture_apply -- <out>/lost<iter>_<ds>.bin holds k int32 rows and k records, <out>/losses.txt `iter n_lost n_left`, and the
snapshots shrink.  The rule has no tolerance (tests/aperture_numpy.py): files are compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import aperture_numpy as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
HALF = (0.0075, 0.0025, 0.025)          # 2.5 rms radii of the reference Gaussian (sigma = 0.003, 0.001, 0.01)
FAR = (3.0, 1.0, 10.0)                  # 1e3 rms radii: nobody gets there


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


def losses(folder):
    return [tuple(int(v) for v in line.split()) for line in (folder / "losses.txt").read_text().splitlines()]


def read_lost(path, width, dtype):
    """(ids, records) of a loss file: k int32, then k x width values of dtype"""
    raw = path.read_bytes()
    k, rest = divmod(len(raw), 4 + width * np.dtype(dtype).itemsize)
    assert rest == 0, len(raw)
    return np.frombuffer(raw, dtype=np.int32, count=k), np.frombuffer(raw, dtype=dtype, offset=4 * k).reshape(k, width)


def read_snap(path, dim, dtype):
    a = np.fromfile(path, dtype=dtype)
    assert a.size % (2 * dim) == 0
    return a.reshape(2, -1, dim)


def test_help_names_the_flags(nbco3):
    r = run(nbco3, "-h")
    assert r.returncode == 0
    for text in ("-aperture <ellipsoid|box> <hx> <hy> <hz>", "-aperture-centre <cx> <cy> <cz>", "lost<iter>_<ds>.bin", "losses.txt"):
        assert text in r.stdout, text
    r = run(os.path.join(HOST, "nbco"), "-h")
    assert r.returncode == 0 and "-aperture <ellipse|box> <hx> <hy>" in r.stdout and "losses.txt" in r.stdout


def test_refusals(nbco3, tmp_path):
    ap = ["-aperture", "ellipsoid", *HALF]
    for mode in (["-test"], ["-test2"], ["-accuracy", 0.01]):
        r = run(nbco3, "-n", 64, *mode, *ap, "-o", tmp_path)
        assert r.returncode != 0 and "-aperture" in r.stderr, mode
    for bad in (("sphere", 1, 1, 1), ("box", 0, 1, 1), ("box", 1, -1, 1), ("ellipsoid", 1, 1, "nan")):
        r = run(nbco3, "-cpu", "-n", 16, "-aperture", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-aperture" in r.stderr, bad
    assert run(nbco3, "-cpu", "-n", 16, "-aperture", "box", 1, 1).returncode != 0
    r = run(nbco3, "-cpu", "-n", 16, *ap, "-aperture-centre", 0, "inf", 0, "-o", tmp_path)
    assert r.returncode != 0 and "-aperture-centre" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("lost")]
    nbco = os.path.join(HOST, "nbco")
    r = run(nbco, "-n", 64, "-test", "-aperture", "ellipse", 1, 1, "-o", tmp_path)
    assert r.returncode != 0 and "-aperture" in r.stderr
    for bad in (("ellipsoid", 1, 1), ("box", 0, 1), ("ellipse", 1, "nan")):
        r = run(nbco, "-n", 64, "-aperture", *bad, "-o", tmp_path)
        assert r.returncode != 0 and "-aperture" in r.stderr, bad


CPU = ["-cpu", "-cpu-threads", 3, "-n", 512, "-ds", 0.05, "-iters", 20, "-steps", 10]
CPU_ITERS = (0, 10, 20)


def name(kind, it, ds="0.050000"):
    return "%s%d_%s.bin" % (kind, it, ds)


def test_cpu_run_loses_what_the_model_loses(nbco3, oracle32, tmp_path):
    """n = 512, the 2.5-rms ellipsoid, ds = 0.05 with a snapshot every 10 steps: 46 particles are outside after the first step, and
    within a fifth of the trap's period most of the rest follows (counted here with -cpu: 46, 295 and 109 at the three snapshots).
    Snapshot 0 is the plain run's snapshot 0 split by the model; the whole trajectory is the oracle's direct3 leapfrog with the
    model applied at the snapshot iterations, bit for bit."""
    from oracle.pyoracle import KIND_DIRECT3, SCHEME_LEAPFROG
    n = 512
    plain = run_ok(nbco3, tmp_path / "plain", *CPU)
    cut = run_ok(nbco3, tmp_path / "cut", *CPU, "-aperture", "ellipsoid", *HALF)
    assert "-aperture" in (cut / "args.txt").read_text().split()
    rows = losses(cut)
    assert [r[0] for r in rows] == list(CPU_ITERS)
    assert 0 < rows[0][1] < n and any(r[1] > rows[0][1] for r in rows[1:]) and rows[-1][2] > 0      # the choice of ds, steps and iters
    left = n
    for it, n_lost, n_left in rows:
        snap = read_snap(cut / name("out", it), 3, np.float32)
        ids, recs = read_lost(cut / name("lost", it), 6, np.float32)
        assert snap.shape[1] == n_left and len(ids) == n_lost and left == n_left + n_lost
        assert AP.inside(snap[0], AP.ELLIPSOID, HALF).all() and not AP.inside(recs[:, :3], AP.ELLIPSOID, HALF).any()
        assert np.all(np.diff(ids) > 0) and (n_lost == 0 or (0 <= ids[0] and ids[-1] < left))
        left = n_left
    # snapshot 0: nobody has left before, so rows are particle numbers
    first = read_snap(plain / name("out", 0), 3, np.float32)
    keep = AP.inside(first[0], AP.ELLIPSOID, HALF)
    ids, recs = read_lost(cut / name("lost", 0), 6, np.float32)
    assert np.array_equal(ids, np.nonzero(~keep)[0])
    assert recs.tobytes() == np.concatenate([first[0][~keep], first[1][~keep]], axis=1).tobytes()
    assert read_snap(cut / name("out", 0), 3, np.float32).tobytes() == first[:, keep].tobytes()
    # the trajectory
    buf = oracle32.init_reference(n)
    par = oracle32.params(n)                 # xi / N0 throughout: the charge per particle does not change
    oracle32.compute_force(KIND_DIRECT3, buf, par, threads=2)
    for it in range(CPU_ITERS[-1] + 1):
        oracle32.integrate(SCHEME_LEAPFROG, KIND_DIRECT3, buf, par, float(np.float32(0.05)), threads=2)
        if it in CPU_ITERS:
            buf, lost, lost_rows = AP.apply(buf, AP.ELLIPSOID, HALF)
            ids, recs = read_lost(cut / name("lost", it), 6, np.float32)
            assert np.array_equal(ids, lost_rows) and recs.tobytes() == lost.tobytes(), it
            assert (cut / name("out", it)).read_bytes() == buf[:2].tobytes(), it


def test_cpu_box_with_an_open_axis_and_a_centre(nbco3, tmp_path):
    """a slab |x - 0.001| <= 0.004, y and z open: the files follow the model with that centre"""
    half, centre = (0.004, np.inf, np.inf), (0.001, 0.0, 0.0)
    plain = run_ok(nbco3, tmp_path / "plain", *CPU[:-4], "-iters", 0, "-steps", 1)
    cut = run_ok(nbco3, tmp_path / "cut", *CPU[:-4], "-iters", 0, "-steps", 1, "-aperture", "box", 0.004, "inf", "inf", "-aperture-centre", *centre)
    first = read_snap(plain / name("out", 0), 3, np.float32)
    keep = AP.inside(first[0], AP.BOX, half, centre)
    assert 0 < keep.sum() < len(keep)
    ids, _ = read_lost(cut / name("lost", 0), 6, np.float32)
    assert np.array_equal(ids, np.nonzero(~keep)[0])
    assert read_snap(cut / name("out", 0), 3, np.float32).tobytes() == first[:, keep].tobytes()


def test_cpu_far_aperture_changes_nothing(nbco3, tmp_path):
    plain = run_ok(nbco3, tmp_path / "plain", *CPU)
    far = run_ok(nbco3, tmp_path / "far", *CPU, "-aperture", "ellipsoid", *FAR)
    for it in CPU_ITERS:
        assert (plain / name("out", it)).read_bytes() == (far / name("out", it)).read_bytes()
        assert (far / name("lost", it)).read_bytes() == b""
    assert losses(far) == [(it, 0, 512) for it in CPU_ITERS]
    assert not [f for f in os.listdir(plain) if f.startswith("lost") or f == "losses.txt"]


def test_cpu_run_that_loses_everybody_stops(nbco3, tmp_path):
    tmp = tmp_path / "none"
    tmp.mkdir()
    r = run(nbco3, *CPU, "-aperture", "box", 1e-12, 1e-12, 1e-12, "-o", tmp)
    assert r.returncode != 0 and "aperture" in r.stderr
    ids, recs = read_lost(tmp / name("lost", 0), 6, np.float32)
    assert np.array_equal(ids, np.arange(512)) and losses(tmp) == [(0, 512, 0)]
    assert not os.path.exists(tmp / name("out", 10))


# ---- on the GPU: every file equals an Engine replay of the same run ---------------------------------------------------------------
GPU = ["-n", 4096, "-p", 4, "-iters", 4, "-steps", 2]
GPU_ITERS = (0, 2, 4)


def replay3(oracle32, scheme, input_order, half):
    """the run of `nbco3 -n 4096 -p 4 -iters 4 -steps 2 -aperture ellipsoid <half>` through the Engine: {file name: bytes}"""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_FMM_KDTREE, Engine
    n = 4096
    files = {}
    e = Engine(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, sync=0, track_order=int(input_order))
    try:
        d = torch.from_numpy(oracle32.init_reference(n).copy()).cuda().reshape(-1)
        prm = torch.from_numpy(oracle32.params(n)).cuda()
        lost = torch.zeros(6 * n, dtype=torch.float32, device="cuda")
        lost_row = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        for it in range(GPU_ITERS[-1] + 1):
            e.integrate_steps(scheme, EVAL_FMM_KDTREE, d, n, prm, float(np.float32(5e-4)), 1)
            if it not in GPU_ITERS:
                continue
            e.sync()
            order = e.kd_array("order") if input_order else None
            kept = e.aperture(d, n, AP_ELLIPSOID, half, lost=lost, lost_row=lost_row)
            k = n - kept
            ids = lost_row[:k].cpu().numpy()
            recs = lost[:6 * k].cpu().numpy()
            snap = d[:6 * kept].cpu().numpy().reshape(2, kept, 3)
            if input_order:
                gone = np.zeros(n, dtype=bool)
                gone[ids] = True
                ids, order = order[ids], order[~gone]
                snap = snap[:, np.argsort(order, kind="stable")]
            files[name("lost", it, "0.000500")] = ids.astype(np.int32).tobytes() + recs.tobytes()
            files[name("out", it, "0.000500")] = np.ascontiguousarray(snap).tobytes()
            n = kept
    finally:
        e.close()
    return files


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["leapfrog", "pefrl", "input"])
def test_gpu_files_are_the_engine_replay(nbco3, oracle32, tmp_path, variant):
    from coulomb_oscillators_amd import INTEG_LEAPFROG, INTEG_PEFRL
    extra = {"leapfrog": [], "pefrl": ["-integ", "pefrl"], "input": ["-snapshot-order", "input"]}[variant]
    cut = run_ok(nbco3, tmp_path / "cut", *GPU, *extra, "-aperture", "ellipsoid", *HALF)
    want = replay3(oracle32, INTEG_PEFRL if variant == "pefrl" else INTEG_LEAPFROG, variant == "input", HALF)
    rows = losses(cut)
    assert [r[0] for r in rows] == list(GPU_ITERS) and 0 < rows[0][1] < 4096
    for fname, data in want.items():
        assert (cut / fname).read_bytes() == data, fname
    assert sorted(f for f in os.listdir(cut) if f.endswith(".bin")) == sorted(want)
    left = 4096
    for it, n_lost, n_left in rows:
        assert left == n_left + n_lost and os.path.getsize(cut / name("out", it, "0.000500")) == 24 * n_left
        left = n_left


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["leapfrog", "input"])
def test_gpu_far_aperture_changes_nothing(nbco3, tmp_path, variant):
    extra = ["-snapshot-order", "input"] if variant == "input" else []
    plain = run_ok(nbco3, tmp_path / "plain", *GPU, *extra)
    far = run_ok(nbco3, tmp_path / "far", *GPU, *extra, "-aperture", "ellipsoid", *FAR)
    for it in GPU_ITERS:
        assert (plain / name("out", it, "0.000500")).read_bytes() == (far / name("out", it, "0.000500")).read_bytes()
        assert (far / name("lost", it, "0.000500")).read_bytes() == b""
    assert losses(far) == [(it, 0, 4096) for it in GPU_ITERS]


@pytest.mark.gpu
def test_gpu_2d_files_are_the_engine_replay(nbco3, oracle32, tmp_path):
    """`nbco -aperture ellipse ..` on an input file (the xy columns of the reference Gaussian as doubles): the same, with fp64 rows of 4"""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL2D_FMM, INTEG_LEAPFROG, Engine
    nbco = os.path.join(HOST, "nbco")
    n = n0 = 4096
    ref = oracle32.init_reference(n)
    state = np.ascontiguousarray(ref[:2, :, :2].astype(np.float64))
    state.tofile(tmp_path / "in.bin")
    args = ["-xi", 2e-6, "-omega0", 1.095, 1.0, "-iters", 4, "-steps", 2]
    cut = run_ok(nbco, tmp_path / "cut", *args, "-aperture", "ellipse", *HALF[:2], tmp_path / "in.bin")
    plain = run_ok(nbco, tmp_path / "plain", *args, tmp_path / "in.bin")
    far = run_ok(nbco, tmp_path / "far", *args, "-aperture", "box", *FAR[:2], tmp_path / "in.bin")
    for it in GPU_ITERS:
        assert (plain / name("out", it, "0.000500")).read_bytes() == (far / name("out", it, "0.000500")).read_bytes()
        assert (far / name("lost", it, "0.000500")).read_bytes() == b""
    e = Engine(fmm_order=5, sync=0)
    try:
        d = torch.zeros(6 * n, dtype=torch.float64, device="cuda")
        d[:4 * n] = torch.from_numpy(state.reshape(-1)).cuda()
        prm = torch.tensor([2e-6 / n, 0.0, 1.095 * 1.095, 1.0 * 1.0], dtype=torch.float64, device="cuda")
        lost = torch.zeros(4 * n, dtype=torch.float64, device="cuda")
        lost_row = torch.zeros(n, dtype=torch.int32, device="cuda")
        e.compute_force_2d(EVAL2D_FMM, d, n, prm)
        rows = []
        for it in range(GPU_ITERS[-1] + 1):
            e.integrate_2d(INTEG_LEAPFROG, EVAL2D_FMM, d, n, prm, 5e-4)
            if it not in GPU_ITERS:
                continue
            kept = e.aperture_2d(d, n, AP_ELLIPSOID, HALF[:2], lost=lost, lost_row=lost_row)
            k = n - kept
            assert (cut / name("lost", it, "0.000500")).read_bytes() == lost_row[:k].cpu().numpy().tobytes() + lost[:4 * k].cpu().numpy().tobytes(), it
            assert (cut / name("out", it, "0.000500")).read_bytes() == d[:4 * kept].cpu().numpy().tobytes(), it
            rows.append((it, k, kept))
            n = kept
    finally:
        e.close()
    assert losses(cut) == rows and 0 < rows[0][1] < n0
