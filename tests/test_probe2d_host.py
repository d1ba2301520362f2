"""The yardsticks of the 2-D probe calls without a GPU: tests/probe2d_numpy.py by its own properties (closed forms, and the FMM
restatement's distance from the exact sum against the field FMM's at the same order), and the `nbco -probes` flag in the help text."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import fmm2d_numpy as F
import probe2d_numpy as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBCO = os.path.join(ROOT, "coulomb_oscillators_amd", "host", "nbco")
EPS2_F32 = float(np.float32(1e-18))
ORDERS = (1, 3, 5, 7, 10)


@pytest.fixture(scope="module", autouse=True)
def the_probe_calls_exist(engine_lib):
    """the yardsticks of this file belong to two entry points; a library without them has nothing to hold to these"""
    lib = ctypes.CDLL(engine_lib)
    assert hasattr(lib, "nbco_2d_probe") and hasattr(lib, "nbco_2d_probe_fmm")


def _closed(src, t, n, eps2, p0):
    d = t - src
    r2 = (d * d).sum(1) + eps2
    return n * p0 * d / r2[:, None], -n * p0 * 0.5 * np.log(r2)


def _both(x, t, p, eps2, p0):
    a, psi, _ab = PR.exact(x, t, eps2, p0)
    return (a, psi), PR.fmm(x, t, p, eps2, p0)


def _close(got, want, rtol=1e-13):
    return np.abs(got - want).max() <= rtol * np.abs(want).max()


def test_one_source_gives_the_pair_law():
    """a = param[0] d / (|d|^2 + EPS2), psi = -param[0] 1/2 log(|d|^2 + EPS2): one source is its own centroid, so every multipole
    above the monopole vanishes and the far field is the pair law too"""
    x = np.array([[0.3, -0.2]])
    rng = np.random.default_rng(0)
    t = np.concatenate([x, x + rng.normal(size=(40, 2)), x + 100 * rng.normal(size=(10, 2)), x + 1e-4 * rng.normal(size=(10, 2))])
    for eps2 in (1e-6, EPS2_F32):
        wa, wp = _closed(x[0], t, 1, eps2, 0.7)
        for p in (1, 5, 10):
            for a, psi in _both(x, t, p, eps2, 0.7):
                assert _close(a, wa) and _close(psi, wp), (eps2, p)
                assert a[0, 0] == 0.0 and a[0, 1] == 0.0   # a probe on top of a source gets nothing from it


def test_coincident_sources_give_n_times_the_pair_law():
    """300 sources at one point with EPS2 = 1e-6 (the cell size is clamped at sqrt(EPS2)): n times the pair law at probes on the
    point, next to it, across the box of cells and far outside it"""
    n, eps2 = 300, 1e-6
    x = F.shape("all_coincident", n)[0]
    rng = np.random.default_rng(1)
    t = np.concatenate([x[:3], x[0] + 1e-3 * rng.normal(size=(50, 2)), x[0] + rng.uniform(0, 0.03, size=(50, 2)), x[0] + rng.normal(size=(20, 2))])
    wa, wp = _closed(x[0], t, n, eps2, 1.0 / n)
    for p in (1, 5, 10):
        for a, psi in _both(x, t, p, eps2, 1.0 / n):
            assert _close(a, wa) and _close(psi, wp), p
            assert np.array_equal(a[:3], np.zeros((3, 2)))


@functools.lru_cache(maxsize=None)
def _kv(n):
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _ = F.kv_params()
    return init2d(n, "kv", A, om)


def probe_sets(x, seed=0):
    """the four probe sets of the KV tests: every 10th particle, 400 uniform points in the bounding box, 400 in a square 1.5 x the
    box's larger half-width about its centre, 200 in a square 10 x that"""
    rng = np.random.default_rng(seed)
    mn, mx = x.min(0), x.max(0)
    ctr, half = (mn + mx) / 2, (mx - mn).max() / 2
    return {"particles": x[::10].copy(), "box": rng.uniform(mn, mx, size=(400, 2)),
            "x1.5": ctr + rng.uniform(-1.5 * half, 1.5 * half, size=(400, 2)), "x10": ctr + rng.uniform(-10 * half, 10 * half, size=(200, 2))}


def _mean_rel(a, ref):
    return float(np.mean(np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)))


@pytest.mark.parametrize("p", ORDERS)
def test_restatement_is_closer_to_the_exact_sum_than_the_field_fmm(engine_lib, p):
    """KV 6000: over each probe set the mean of |a - exact| / |exact| is no larger than the same mean of fmm2d_numpy.fmm against
    fmm2d_numpy.direct on the particles at that order -- the probes skip the second truncation of the locals, and a point outside
    the sources' square is farther from every source than its projection.  Measured here (field FMM | particles, box, x1.5, x10):
      p = 1   7.81e-2 | 4.83e-3 3.85e-3 1.86e-3 1.43e-4        p = 7   8.05e-6 | 4.94e-6 4.50e-6 1.47e-6 1.64e-7
      p = 3   3.12e-3 | 3.14e-4 2.69e-4 1.32e-4 1.04e-5        p = 10  3.56e-7 | 2.11e-7 1.73e-7 8.76e-8 6.70e-9
      p = 5   8.43e-5 | 2.44e-5 1.90e-5 7.63e-6 3.90e-7
    The potential's distance, relative to max |psi| of the set, is printed with them."""
    st = _kv(6000)
    x = st[0]
    _A, _om, xi, _om0 = F.kv_params()
    p0 = xi / 6000
    _s, a_f = F.fmm(st, p, EPS2_F32, [p0, 0.0])
    order = np.argsort(F.keys(x, F.levels(6000, p), EPS2_F32), kind="stable")
    bound = _mean_rel(a_f, F.direct(x[order], EPS2_F32, p0))
    for name, t in probe_sets(x).items():
        ea, epsi, _ab = PR.exact(x, t, EPS2_F32, p0)
        a, psi = PR.fmm(x, t, p, EPS2_F32, p0)
        err = _mean_rel(a, ea)
        print("p=%d %s: probes %.3e field fmm %.3e, psi %.3e of max |psi|" % (p, name, err, bound, np.abs(psi - epsi).max() / np.abs(epsi).max()))
        assert err <= bound, (p, name, err, bound)


@pytest.fixture(scope="module")
def nbco(engine_lib):
    if not os.path.exists(NBCO):
        subprocess.check_call(["make", "-C", os.path.dirname(NBCO), "-s", "nbco"])
    return NBCO


def test_help_mentions_the_probes_flag(nbco):
    r = subprocess.run([nbco, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "-probes" in r.stdout and "probes<iter>_<ds>.bin" in r.stdout
