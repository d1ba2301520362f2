"""The Langevin bath without a GPU: the Philox model of tests/bath_numpy.py against known answers, nbco_bath_coeffs against a
long-double model, the model's statistics (free particles, a harmonic trap under leapfrog), argument errors, and `nbco3 -cpu -bath`
against the model byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bath_numpy as bn
import integrators3d_numpy as ig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib(engine_lib):
    import coulomb_oscillators_amd as co
    return co


# ---- the noise ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, out in bn.KNOWN_ANSWERS:
        got = tuple(int(w) for w in bn.philox4x32_10(ctr, key))
        assert got == out, (ctr, key, [hex(w) for w in got])
    # arrays go through the same arithmetic as scalars
    ctr = np.array([c for c, _, _ in bn.KNOWN_ANSWERS[:1] * 3 + bn.KNOWN_ANSWERS[1:2]], dtype=np.uint64).T
    w = bn.philox4x32_10(tuple(ctr), (0, 0))
    assert tuple(int(q[0]) for q in w) == bn.KNOWN_ANSWERS[0][2] and w[0].shape == (4,)


def test_noise_moments_and_range():
    """a centred sum of four uniforms: mean 0, variance 1, kurtosis 2.7, |xi| <= 2 sqrt(3) = 3.47.  At n = 65536 the mean is within five
    standard errors (5 / sqrt(n)), the variance within 5 sqrt((2.7 - 1) / n), the kurtosis within 0.15 of 2.7 (its standard error at a
    bounded distribution like this one is about 0.02)."""
    n = 65536
    x = bn.xi(12345, 7, 1, np.arange(n), 2)
    var = x.var()
    print("mean %.4f variance %.4f kurtosis %.3f max %.3f" % (x.mean(), var, ((x - x.mean()) ** 4).mean() / var ** 2, np.abs(x).max()))
    assert abs(x.mean()) <= 5 / np.sqrt(n)
    assert abs(var - 1) <= 5 * np.sqrt(1.7 / n)
    assert abs(((x - x.mean()) ** 4).mean() / var ** 2 - 2.7) <= 0.15
    assert np.abs(x).max() <= 2 * np.sqrt(3)
    # every word of the counter and the key enters: the streams differ, and a stream is reproducible
    base = bn.xi(12345, 7, 1, np.arange(64), 2)
    assert np.array_equal(base, bn.xi(12345, 7, 1, np.arange(64), 2))
    for other in (bn.xi(12346, 7, 1, np.arange(64), 2), bn.xi(12345 + (1 << 32), 7, 1, np.arange(64), 2), bn.xi(12345, 8, 1, np.arange(64), 2),
                  bn.xi(12345, 7 + (1 << 32), 1, np.arange(64), 2), bn.xi(12345, 7, 0, np.arange(64), 2), bn.xi(12345, 7, 1, np.arange(64), 1),
                  bn.xi(12345, 7, 1, np.arange(1, 65), 2)):
        assert not np.array_equal(base, other)
    # the extremes of the sum map to -+2 sqrt(3) (1 - 2^-32 ..), the centre to 0
    assert (0 - bn.XI_CENTRE) * bn.XI_SCALE == -(4 * 0xFFFFFFFF - bn.XI_CENTRE) * bn.XI_SCALE


# ---- the coefficients -----------------------------------------------------------------------------------------------------------
def test_coeffs_against_long_double(lib):
    """c1 = exp(-gamma s) within 2 ulp; c2 = sqrt(kT (1 - exp(-2 gamma s))) within 4 ulp (exp or expm1, one product, one root, and the
    rounding of gamma s that the exponential passes on: |gamma s| eps relative, which the bound adds)"""
    worst = 0.0
    for gamma in (0.0, 1e-12, 1e-3, 0.3, 1.0, 7.0, 40.0, 1e3):
        for s in (0.0, 1e-6, 0.25, 0.5, 1.0, 3.0):
            for kT in (0.0, 1e-8, 0.5, 1.0, 2.0, 1e6):
                c1, c2 = lib.bath_coeffs((gamma, 0.5 * gamma, 0.0), (kT, 2 * kT, kT), s)
                m1, m2 = bn.coeffs_ld((gamma, 0.5 * gamma, 0.0), (kT, 2 * kT, kT), s)
                for a in range(3):
                    g = (gamma, 0.5 * gamma, 0.0)[a]
                    slack = 1 + g * s
                    for got, want, ulps in ((c1[a], m1[a], 2), (c2[a], m2[a], 4)):
                        err = abs(np.longdouble(got) - want)
                        bound = ulps * slack * np.spacing(np.float64(want)) if want != 0 else 0.0
                        worst = max(worst, float(err / bound) if bound else float(err))
                        assert err <= bound, (gamma, s, kT, a, got, float(want))
                assert c1[2] == 1.0 and c2[2] == 0.0                      # gamma = 0: exactly 1 and 0
    print("worst error: %.2f of the bound" % worst)


def test_coeffs_argument_errors(lib):
    for gamma, kT, s in (((-1, 0, 0), (1, 1, 1), 0.5), ((np.nan, 0, 0), (1, 1, 1), 0.5), ((0, np.inf, 0), (1, 1, 1), 0.5), ((1, 1, 1), (0, -1e-9, 0), 0.5),
                         ((1, 1, 1), (0, 0, np.nan), 0.5), ((1, 1, 1), (1, 1, 1), -0.5), ((1, 1, 1), (1, 1, 1), np.inf), ((1, 1, 1), (1, 1, 1), np.nan)):
        with pytest.raises(lib.EngineError) as ei:
            lib.bath_coeffs(gamma, kT, s)
        assert ei.value.status == 2
    from coulomb_oscillators_amd.engine import _load, Bath
    L = _load()
    c = (C.c_double * 3)()
    b = Bath((C.c_double * 3)(1, 1, 1), (C.c_double * 3)(1, 1, 1), 1)
    assert L.nbco_bath_coeffs(None, 0.5, c, c) == 2 and L.nbco_bath_coeffs(C.byref(b), 0.5, None, c) == 2 and L.nbco_bath_coeffs(C.byref(b), 0.5, c, None) == 2
    # a null context is refused by every device call without touching anything
    assert L.nbco_bath_apply(None, None, 1, C.byref(b), 0.5, 0, 0) == 2
    assert L.nbco_integrate_t(None, 2, 0, None, 1, None, 0.1, 1.0, 1, None, C.byref(b), 0) == 2
    assert L.nbco_2d_integrate_steps_t(None, 2, 0, None, 1, None, 0.1, 1.0, 1, 2, 0.0, C.byref(b), 0) == 2


# ---- the model's statistics -----------------------------------------------------------------------------------------------------
def test_free_particles_variance_recursion_and_pure_cooling(lib):
    """free particles: one O step takes the variance sigma^2 to c1^2 sigma^2 + c2^2 (within five standard errors of the sampled
    variance, 5 sqrt(2 / n) relative at a kurtosis of at most 3); with kT = 0, K steps multiply v by c1^(2K) to rounding"""
    n, dt = 65536, 0.5
    gamma, kT = (1.0, 0.3, 0.0), (0.5, 1.0, 2.0)
    bath = bn.Bath(gamma, kT, 99, coeffs=lib.bath_coeffs)
    c1, c2 = lib.bath_coeffs(gamma, kT, 0.5 * dt)
    rng = np.random.default_rng(3)
    v0 = rng.normal(size=(n, 3)) * np.array([0.5, 2.0, 1.5])
    v1 = bath.half_step(v0, dt, 11, 0)
    for a in range(3):
        want = c1[a] ** 2 * v0[:, a].var() + c2[a] ** 2
        got = v1[:, a].var()
        print("axis %d: variance %.4f -> %.4f, recursion %.4f" % (a, v0[:, a].var(), got, want))
        assert abs(got / want - 1) <= 5 * np.sqrt(2.0 / n)
    assert np.array_equal(v1[:, 2], v0[:, 2])                             # gamma = 0: the axis is left alone
    cold = bn.Bath(gamma, (0.0, 0.0, 0.0), 99, coeffs=lib.bath_coeffs)
    K = 9
    vK = bn.free_bath_run(v0, dt, K, cold)
    for a in range(3):
        assert np.abs(vK[:, a] - c1[a] ** (2 * K) * v0[:, a]).max() <= 4 * K * EPS * np.abs(v0[:, a]).max()


def _trap_covariance(k, dt, gamma, kT, lib):
    """stationary covariance of (x, v) of one particle in a = -k x under leapfrog with the bath, measured in the model: the model's step
    is linear in (x, v, noise), so its matrix M is read off by stepping unit vectors with kT = 0 (no noise), and the noise's share by
    stepping the zero state with each of the two noises of a step set to one in turn; then Sigma <- M Sigma M^T + sum n n^T to its fixed point"""
    f = ig.elastic_force(np.array([k]))
    cold = bn.Bath((gamma,), (0.0,), 1, coeffs=lambda g, t, s: tuple(c[:1] for c in lib.bath_coeffs(g + (0, 0), t + (0, 0), s)))

    def step(x, v):
        x, v = np.array([[x]]), np.array([[v]])
        xn, vn, _ = bn.integrate(ig.LEAPFROG, f, x, v, f(x), dt, cold, 0)
        return np.array([xn[0, 0], vn[0, 0]])
    M = np.stack([step(1.0, 0.0), step(0.0, 1.0)], axis=1)
    c2 = lib.bath_coeffs((gamma, 0, 0), (kT, 0, 0), 0.5 * dt)[1][0]
    c1 = lib.bath_coeffs((gamma, 0, 0), (kT, 0, 0), 0.5 * dt)[0][0]
    # opening noise: v gets c2 before S and the closing friction, i.e. M applied to (0, c2 / c1) -- M's velocity column carries the
    # opening c1, which the noise does not see; closing noise: added to v after everything
    n_open = M @ np.array([0.0, c2 / c1])
    n_close = np.array([0.0, c2])
    Q = np.outer(n_open, n_open) + np.outer(n_close, n_close)
    S = np.zeros((2, 2))
    for _ in range(100000):
        S2 = M @ S @ M.T + Q
        if np.abs(S2 - S).max() <= 1e-15 * np.abs(S2).max():
            break
        S = S2
    return S2


def test_harmonic_trap_under_leapfrog(lib):
    """<v^2> tends to kT; <k x^2> is shifted at order dt^2 only: the shift measured at dt and at dt / 2 has the ratio 4 (within 5 %: the
    next order is k dt^2 / 4 = 1 % relative at the larger step), at two friction rates.  A sampled run of the model agrees with the
    measured covariance within five standard errors."""
    k, kT = 1.3, 0.7
    for gamma in (0.5, 3.0):
        shifts = []
        for dt in (0.2, 0.1, 0.05):
            S = _trap_covariance(k, dt, gamma, kT, lib)
            print("gamma %.1f dt %.2f: <v^2>/kT - 1 = %+.2e, <k x^2>/kT - 1 = %+.3e, <x v> = %+.1e" % (gamma, dt, S[1, 1] / kT - 1, k * S[0, 0] / kT - 1, S[0, 1]))
            assert abs(S[1, 1] / kT - 1) <= 1e-9
            shifts.append(k * S[0, 0] / kT - 1)
        assert all(s > 0 for s in shifts) and shifts[0] < 0.02
        for big, small in zip(shifts, shifts[1:]):
            assert abs(big / small / 4 - 1) <= 0.05, shifts
    # the sampled model: n independent particles (one per row) from a cold start, 60 steps at gamma dt = 0.6
    n, dt, gamma, steps = 65536, 0.2, 3.0, 60
    bath = bn.Bath((gamma,), (kT,), 2024, coeffs=lambda g, t, s: tuple(c[:1] for c in lib.bath_coeffs(g + (0, 0), t + (0, 0), s)))
    f = ig.elastic_force(np.array([k]))
    x, v, _ = bn.run(ig.LEAPFROG, f, np.zeros((n, 1)), np.zeros((n, 1)), dt, steps, bath)[-1]
    S = _trap_covariance(k, dt, gamma, kT, lib)
    print("sampled: <v^2> %.4f (model %.4f), <x^2> %.4f (model %.4f)" % ((v * v).mean(), S[1, 1], (x * x).mean(), S[0, 0]))
    assert abs((v * v).mean() / S[1, 1] - 1) <= 5 * np.sqrt(2.0 / n)
    assert abs((x * x).mean() / S[0, 0] - 1) <= 5 * np.sqrt(2.0 / n)


def test_model_without_bath_is_the_plain_scheme():
    rng = np.random.default_rng(5)
    x, v = rng.normal(size=(2, 7, 3))
    f = ig.elastic_force(np.array([1.2, 1.0, 0.7]))
    off = bn.Bath((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), 5)
    for scheme in ig.SCHEMES:
        want = ig.integrate(scheme, f, x, v, f(x), 0.37, 0.5)
        got = bn.integrate(scheme, f, x, v, f(x), 0.37, off, 3, scale=0.5)
        for g, w in zip(got, want):
            assert np.abs(g - w).max() < 1e-14


# ---- nbco3 -cpu -bath -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco3(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "nbco3")


@pytest.mark.parametrize("name,flags,scheme", [("leapfrog", [], ig.LEAPFROG), ("eu", ["-integ", "eu"], ig.EULER)])
def test_nbco3_cpu_with_bath_is_the_model_byte_for_byte(lib, nbco3, oracle32, tmp_path, name, flags, scheme):
    """`nbco3 -cpu -bath` at n = 64 with the Coulomb sum switched off (-xi 0: the force is the trap alone, a = -(k o x) in float32, which
    numpy restates exactly; the step coefficients of the two schemes are dt and dt / 2, exact in every precision): every snapshot's bytes
    are those of the float32 model, the tick of an iteration its number.  The z axis has gamma = 0, the y axis kT = 0."""
    n, iters = 64, 4
    out = tmp_path / "out"
    out.mkdir()
    bath = ("0.8", "2.5", "0", "0.5", "0", "2")
    args = [nbco3, "-cpu", "-n", str(n), "-ds", "0.05", "-iters", str(iters), "-steps", "2", "-xi", "0", "-bath", *bath, "-bath-seed", "81985529216486895",
            "-o", str(out)] + flags
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "-bath 0.8 2.5 0 0.5 0 2" in (out / "args.txt").read_text()
    dt = float(np.float32(0.05))
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    k = par[3:6].astype(np.float32)
    force = lambda x: -(x * k)
    model = bn.Bath(tuple(float(q) for q in bath[:3]), tuple(float(q) for q in bath[3:]), 81985529216486895, coeffs=lib.bath_coeffs)
    states = bn.run(scheme, force, buf[0], buf[1], dt, iters + 1, model, dtype=np.float32)
    for snap in (0, 2, 4):
        got = np.fromfile(out / ("out%d_%s.bin" % (snap, "%.6f" % dt)), dtype=np.float32).reshape(2, n, 3)
        for q in range(2):
            assert got[q].tobytes() == states[snap][q].tobytes(), (name, snap, q, np.abs(got[q] - states[snap][q]).max())
    # and the bath does something: the run without it ends elsewhere
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([a for a in args[:args.index("-bath")]] + ["-o", str(plain)] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (plain / ("out4_%s.bin" % ("%.6f" % dt))).read_bytes() != (out / ("out4_%s.bin" % ("%.6f" % dt))).read_bytes()


def test_nbco3_cpu_zero_rates_are_the_run_without_the_flag(nbco3, tmp_path):
    snaps = []
    for extra in ([], ["-bath", "0", "0", "0", "1", "2", "3"], ["-bath", "0", "-0", "0.0", "0", "0", "0", "-bath-seed", "7"]):
        out = tmp_path / ("o%d" % len(snaps))
        out.mkdir()
        r = subprocess.run([nbco3, "-cpu", "-n", "64", "-ds", "0.05", "-iters", "2", "-steps", "1", "-integ", "pefrl", "-o", str(out)] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        snaps.append((out / "out2_0.050000.bin").read_bytes())
    assert len(snaps[0]) == 64 * 24 and snaps[0] == snaps[1] == snaps[2]


def test_cli_argument_errors(nbco3):
    nbco, dist = os.path.join(HOST, "nbco"), os.path.join(HOST, "nbco3_dist")
    for exe, args, msg in ((nbco3, ["-bath", "1", "2", "3", "4", "5"], "missing argument(s) to '-bath'"), (nbco3, ["-bath", "1", "-1", "0", "1", "1", "1"], "invalid argument(s) to '-bath'"),
                           (nbco3, ["-bath", "1", "1", "0", "1", "nan", "1"], "invalid argument(s) to '-bath'"), (nbco3, ["-bath-seed", "-3"], "invalid argument to '-bath-seed'"),
                           (nbco3, ["-bath-seed", "12x"], "invalid argument to '-bath-seed'"), (nbco, ["-bath", "1", "1", "1"], "missing argument to '-bath'"),
                           (nbco, ["-bath", "1", "inf", "1", "1"], "invalid argument to '-bath'"), (nbco, ["-bath", "1", "1", "1", "-2"], "invalid argument to '-bath'"),
                           (dist, ["-bath", "1", "1", "1", "1", "1", "1"], "'-bath' is not available with kd-domain sharding")):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
    for exe in (nbco3, nbco):
        assert "-bath <gx>" in subprocess.run([exe, "-h"], capture_output=True, text=True, timeout=60).stdout
