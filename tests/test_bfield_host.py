"""The uniform magnetic field without a GPU: nbco_helix_matrices against the long-double model of tests/bfield_numpy.py, the matrices'
own identities, the model's integrators against closed forms (a free particle's helix, one particle in a Penning trap), and
`nbco3 -cpu -B` end to end against the fp64 model."""
import os
import subprocess

import numpy as np
import pytest

import bfield_numpy as bf
import integrators3d_numpy as ig
from direct_numpy import direct_rows_fp64, direct3_rows_fp32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")

SERIES = 0.5       # |theta| below which nbco_helix_matrices sums theta - sin(theta) as a series (include/nbco.h)
THETAS = (0.0, 1e-9, -1e-9, 1e-4, -1e-4, np.nextafter(SERIES, 0), SERIES, -np.nextafter(SERIES, 0), -SERIES, 0.49, 0.51, 1.0, np.pi, 2 * np.pi, 100.0)
AXES = {"x": (0.8, 0, 0), "y": (0, -1.7, 0), "z": (0, 0, 0.31), "oblique": bf.OMEGA, "oblique2": (-2.0, 3.0, 0.001)}
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib(engine_lib):
    import coulomb_oscillators_amd as co
    return co


def _within_ulps(got, want, ulps=4):
    """every element within `ulps` ulp (double) of the largest element of the long-double matrix"""
    bound = ulps * np.spacing(np.float64(np.abs(want).max()))
    err = np.abs(got.astype(np.longdouble) - want).max()
    return float(err), float(bound)


@pytest.mark.parametrize("axis", sorted(AXES))
def test_matrices_against_long_double(lib, axis):
    """4 ulp of the matrix's largest element: a handful of roundings.  s = theta / |Omega| in double and its negative: the angle the
    call sees is |Omega| s, which the model forms from the same two inputs in long double."""
    omega = AXES[axis]
    w = float(np.sqrt(sum(np.longdouble(c) ** 2 for c in omega)))
    worst = 0.0
    for theta in THETAS:
        for s in (theta / w, -theta / w):
            R, A = lib.helix_matrices(omega, s)
            Rm, Am = bf.matrices(omega, s)
            for name, got, want in (("R", R, Rm), ("A", A, Am)):
                err, bound = _within_ulps(got, want)
                worst = max(worst, err / bound if bound else 0.0)
                assert err <= bound, (axis, theta, s, name, err, bound)
    print("%s: worst error %.2f of the 4 ulp bound" % (axis, worst))


def test_matrices_2d_against_long_double(lib):
    """the same bound, plus what the model itself cannot resolve: in the plane nothing is parallel to the field, so at theta = 2 pi
    the whole of A is sin(theta) / w, about 1e-16, and 4 ulp of that is far below the rounding of the model's own long-double angle
    (|theta| 2^-64, which sin and 1 - cos pass on, divided by |w| in A)."""
    for w in (0.31, -1.7, 100.0):
        for theta in THETAS:
            for s in (theta / w, -theta / w):
                R, A = lib.helix_matrices_2d(w, s)
                Rm, Am = bf.matrices_2d(w, s)
                for name, got, want, scale in (("R", R, Rm, 1.0), ("A", A, Am, 1.0 / abs(w))):
                    err, bound = _within_ulps(got, want)
                    bound += 2.0 ** -63 * abs(theta) * scale
                    assert err <= bound, (w, theta, s, name, err, bound)
    # the 2-D matrices are the x-y block of the 3-D ones for a field along z
    R2, A2 = lib.helix_matrices_2d(0.7, 1.3)
    R3, A3 = lib.helix_matrices((0, 0, 0.7), 1.3)
    assert np.abs(R3[:2, :2] - R2).max() <= 4 * EPS and np.abs(A3[:2, :2] - A2).max() <= 4 * 1.3 * EPS


def test_matrix_identities(lib):
    I = np.eye(3)
    for s in (0.0, 1.0, -2.5, 1e-300):
        R, A = lib.helix_matrices((0.0, 0.0, 0.0), s)
        assert np.array_equal(R, I) and np.array_equal(A, s * I)            # w = 0: exactly I and s I
        R, A = lib.helix_matrices_2d(0.0, s)
        assert np.array_equal(R, np.eye(2)) and np.array_equal(A, s * np.eye(2))
    for omega in AXES.values():
        for s1, s2 in ((0.3, 1.1), (-0.7, 2.0), (1e-5, -40.0)):
            R1, _ = lib.helix_matrices(omega, s1)
            R2, _ = lib.helix_matrices(omega, s2)
            R12, _ = lib.helix_matrices(omega, s1 + s2)
            Rm, _ = lib.helix_matrices(omega, -s1)
            w = np.linalg.norm(omega)
            tol = 16 * EPS * (1 + w * (abs(s1) + abs(s2)))                     # (the angle of R(s1 + s2) carries the rounding of the sum)
            assert np.abs(R1.T @ R1 - I).max() <= 8 * EPS
            assert np.abs(R1 @ Rm - I).max() <= 8 * EPS
            assert np.abs(R1 @ R2 - R12).max() <= tol
            # dA/ds = R: central difference, truncation h^2 w^2 / 6 and rounding eps |s| / h
            h = 1e-5
            dA = (lib.helix_matrices(omega, s1 + h)[1] - lib.helix_matrices(omega, s1 - h)[1]) / (2 * h)
            assert np.abs(dA - R1).max() <= 1e-8 * (1 + w * w)
    for bad in ((np.nan, 0, 0), (0, np.inf, 0)):
        with pytest.raises(lib.EngineError):
            lib.helix_matrices(bad, 1.0)
    with pytest.raises(lib.EngineError):
        lib.helix_matrices_2d(np.inf, 1.0)


# ---- the model by closed forms --------------------------------------------------------------------------------------------------
def test_sequences_are_those_of_the_plain_schemes():
    """the traced sequence replays integrators3d_numpy.integrate exactly when the drift is the straight one"""
    rng = np.random.default_rng(5)
    x, v = rng.normal(size=(2, 7, 3))
    k = np.array([1.2, 1.0, 0.7])
    f = ig.elastic_force(k)
    for scheme in ig.SCHEMES:
        seq = bf.sequence(scheme, 0.37, 0.5)
        assert abs(sum(op[1] for op in seq if op[0] == "D") - 0.37) < 1e-15            # the drift coefficients add up to dt
        want = ig.integrate(scheme, f, x, v, f(x), 0.37, 0.5)
        got = bf.integrate(scheme, f, x, v, f(x), 0.37, (0.0, 0.0, 0.0), 0.5)
        for g, w in zip(got, want):
            assert np.abs(g - w).max() < 1e-14


@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_free_particle_gyrates_exactly(scheme):
    """no force: K steps of any scheme are the closed-form helix at K dt, whatever the step"""
    x0, v0 = np.array([[0.1, -0.2, 0.3]]), np.array([[1.0, 0.5, -0.25]])
    zero = lambda x: np.zeros_like(x)
    for dt, steps in ((0.5, 7), (3.0, 4)):
        x, v, _ = bf.run(scheme, zero, x0, v0, dt, steps, bf.OMEGA)[-1]
        xe, ve = bf.free_helix(x0, v0, bf.OMEGA, steps * dt)
        assert np.abs(x - xe).max() < 1e-12 and np.abs(v - ve).max() < 1e-12


KZ, WC, T_PENNING = 1.0, 2.5, 0.5      # wc^2 > 2 kz; half a time unit: a fifth of a cyclotron period, the steps resolve it well


def _penning(scheme, steps, x0, v0, wc=WC):
    k = np.array([-KZ / 2, -KZ / 2, KZ])
    return bf.run(scheme, ig.elastic_force(k), x0, v0, T_PENNING / steps, steps, (0.0, 0.0, wc))[-1]


@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_penning_trap_order_and_reversal(scheme):
    x0, v0 = np.array([[0.3, -0.1, 0.2]]), np.array([[0.2, 0.5, -0.3]])
    xe, ve = bf.penning_orbit(x0[0], v0[0], KZ, WC, T_PENNING)
    errs = []
    for steps in (16, 32, 64):
        x, v, _ = _penning(scheme, steps, x0, v0)
        errs.append(float(np.sqrt(((x[0] - xe) ** 2).sum() + ((v[0] - ve) ** 2).sum())))
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    want = 2.0 ** bf.ORDERS[scheme]
    print(ig.NAMES[scheme], errs, ratios)
    for r in ratios:
        assert abs(r / want - 1) <= 0.25, (errs, ratios, want)
    if scheme in bf.REVERSIBLE:
        # forward, v -> -v and Omega -> -Omega, forward again: back at the start
        x, v, _ = _penning(scheme, 16, x0, v0)
        x, v, _ = _penning(scheme, 16, x, -v, wc=-WC)
        assert np.abs(x - x0).max() < 1e-13 and np.abs(v + v0).max() < 1e-13


# ---- nbco3 -cpu -B --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


CPU_N, CPU_DT, CPU_ITERS = 64, 0.05, 3
CPU_SCHEMES = {"leapfrog": ([], ig.LEAPFROG), "eu": (["-integ", "eu"], ig.EULER), "fr": (["-integ", "fr"], ig.FORESTRUTH), "pefrl": (["-integ", "pefrl"], ig.PEFRL)}


@pytest.mark.parametrize("name", sorted(CPU_SCHEMES))
def test_nbco3_cpu_with_field_against_model(nbco3, oracle32, tmp_path, name):
    """`nbco3 -cpu -B` at n = 64: the last snapshot against the fp64 model (force: the fp64 direct sum and the trap) within
    min(4 x floor, 1e-5), the floor the distance of the float32 emulation (float32 Kahan direct sum, float32 kicks, the emulated
    drift) from the fp64 model.  args.txt echoes the flag."""
    flags, scheme = CPU_SCHEMES[name]
    n = CPU_N
    out = tmp_path / "out"
    out.mkdir()
    omega = ("0.3", "-0.2", "0.7")
    args = [nbco3, "-cpu", "-n", str(n), "-ds", str(CPU_DT), "-iters", str(CPU_ITERS - 1), "-steps", "1", "-B", *omega, "-o", str(out)] + flags
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "-B 0.3 -0.2 0.7" in (out / "args.txt").read_text()
    dt = float(np.float32(CPU_DT))
    snap = np.fromfile(out / ("out%d_%s.bin" % (CPU_ITERS - 1, "%.6f" % dt)), dtype=np.float32).reshape(2, n, 3)
    buf = oracle32.init_reference(n)
    par = oracle32.params(n)
    eps2 = float(np.float32(1e-18))
    rows = np.arange(n)
    k64 = par[3:6].astype(np.float64)
    f64 = lambda x: direct_rows_fp64(x, rows, float(par[0]), eps2) - k64 * x
    f32 = lambda x: direct3_rows_fp32(x.astype(np.float32), rows, par[0], np.float32(eps2)) - par[3:6] * x
    om = tuple(float(w) for w in omega)
    want = bf.run(scheme, f64, buf[0], buf[1], dt, CPU_ITERS, om)[-1]
    emu = bf.run(scheme, f32, buf[0], buf[1], dt, CPU_ITERS, om, f32=True)[-1]
    floor = tuple(ig.rel_dist(emu[q], want[q]) for q in range(2))
    err = tuple(ig.rel_dist(snap[q], want[q]) for q in range(2))
    tol = ig.gpu_tolerance(floor)
    print("%s: floor x %.2e v %.2e   error x %.2e v %.2e   tolerance x %.2e v %.2e" % (name, *floor, *err, *tol))
    assert err[0] <= tol[0] and err[1] <= tol[1], (err, tol)
    # and the field does something: the run without it ends elsewhere
    plain = bf.run(scheme, f64, buf[0], buf[1], dt, CPU_ITERS, (0.0, 0.0, 0.0))[-1]
    assert ig.rel_dist(plain[1], want[1]) > 1e-3


def test_nbco3_cpu_zero_field_is_the_run_without_the_flag(nbco3, tmp_path):
    """`-B 0 0 0` takes the plain drift on the host path too: the same bytes, signed zeros and all"""
    snaps = []
    for extra in ([], ["-B", "0", "0", "0"], ["-B", "-0", "0", "0.0"]):
        out = tmp_path / ("o%d" % len(snaps))
        out.mkdir()
        r = subprocess.run([nbco3, "-cpu", "-n", "64", "-ds", "0.05", "-iters", "2", "-steps", "1", "-integ", "pefrl", "-o", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        snaps.append((out / "out2_0.050000.bin").read_bytes())
    assert len(snaps[0]) == 64 * 24 and snaps[0] == snaps[1] == snaps[2]


def test_cli_argument_errors(nbco3):
    for exe, args, msg in ((nbco3, ["-B", "1", "2"], "missing argument(s) to '-B'"), (nbco3, ["-B", "1", "nan", "0"], "invalid argument(s) to '-B'"),
                           (os.path.join(HOST, "nbco"), ["-B"], "missing argument to '-B'"), (os.path.join(HOST, "nbco"), ["-B", "inf"], "invalid argument to '-B'"),
                           (os.path.join(HOST, "nbco3_dist"), ["-B", "0", "0", "1"], "'-B' is not available with kd-domain sharding")):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
    for exe in (nbco3, os.path.join(HOST, "nbco")):
        assert "-B <w" in subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60).stdout
