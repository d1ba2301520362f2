"""The yardsticks of the 2-D energy diagnostics without a GPU: tests/energy2d_numpy.py by its own properties (closed forms and
convergence towards the exact sum), and the `nbco -energy` flag in the help text."""
import math
import os
import subprocess

import numpy as np
import pytest

import energy2d_numpy as E
import fmm2d_numpy as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBCO = os.path.join(ROOT, "coulomb_oscillators_amd", "host", "nbco")
EPS2_F32 = float(np.float32(1e-18))


def test_all_coincident_particles_give_the_closed_form():
    """n particles at one point: every pair term is 1/2 log EPS2, coulomb = -param[0] / 2 * n (n - 1) / 2 * log EPS2, from the near
    field alone (one occupied leaf, no M2L source), in the exact sum and in the FMM restatement"""
    n, eps2 = 50, 1e-6
    A = np.array(F.kv_params()[0])
    st = np.stack([np.tile(0.25 * A, (n, 1)), np.random.default_rng(0).normal(size=(n, 2))])
    prm = [1.0 / n, 0.0, 1.0, 1.5]
    want = -prm[0] * 0.5 * (n * (n - 1) / 2) * math.log(eps2)
    for p in (1, 5, 10):
        e, psi, S = E.fmm_energy(st, p, eps2, prm)
        assert abs(e[2] - want) <= 1e-13 * abs(want), (p, e[2], want)
        assert np.allclose(psi, 2 * want / n, rtol=1e-13, atol=0)
        assert abs(S - abs(want)) <= 1e-13 * abs(want)
    e, psi, ab = E.exact(st[0], st[1], prm, eps2)
    assert abs(e[2] - want) <= 1e-13 * abs(want)
    assert e[0] == 0.5 * float((st[1] ** 2).sum())


def test_one_particle_has_no_potential_energy():
    st = np.array([[[0.3, -0.2]], [[1.0, 2.0]]])
    prm = [1.0, 0.0, 2.0, 3.0]
    for p in (1, 5):
        e, psi, S = E.fmm_energy(st, p, 1e-6, prm)
        assert e[2] == 0.0 and psi[0] == 0.0 and S == 0.0
        assert e[0] == 2.5 and abs(e[1] - 0.5 * (2.0 * 0.09 + 3.0 * 0.04)) < 1e-16
    assert E.exact(st[0], st[1], prm, 1e-6)[0][2] == 0.0


def _kv(n):
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _ = F.kv_params()
    return init2d(n, "kv", A, om)


def _uniform(n):
    return np.stack([np.random.default_rng(1).uniform(size=(n, 2)), np.zeros((n, 2))])


# measured with this file's inputs at r = 1: the restatement's distance from the exact sum, relative to |coulomb|
#   KV 6000:              p = 3 1.05e-5, p = 5 1.81e-8, p = 7 1.42e-9, p = 10 1.6e-11
#   uniform square 3000:  p = 3 7.49e-5, p = 5 5.32e-8, p = 7 2.74e-8, p = 10 8.6e-11
# the p = 5 bound is twice the measured figure
P5_BOUND = {"kv": 2 * 1.82e-8, "uniform": 2 * 5.32e-8}


@pytest.mark.parametrize("case", ["kv", "uniform"])
def test_restatement_converges_to_the_exact_sum(engine_lib, case):
    st = _kv(6000) if case == "kv" else _uniform(3000)
    n = st.shape[1]
    _A, _om, xi, om0 = F.kv_params()
    prm = [xi / n, 0.0, om0[0] ** 2, om0[1] ** 2]
    ex, psi_x, _ab = E.exact(st[0], st[1], prm, EPS2_F32)
    d = {}
    for p in (3, 5, 7):
        e, psi, S = E.fmm_energy(st, p, EPS2_F32, prm)
        assert e[0] == ex[0] and e[1] == ex[1]
        d[p] = abs(e[2] - ex[2]) / abs(ex[2])
        print("%s p=%d distance %.3e, psi %.3e of max |psi|" % (case, p, d[p], np.abs(psi - psi_x).max() / np.abs(psi_x).max()))
    assert d[7] <= d[3] / 10, d
    assert d[5] <= P5_BOUND[case], d


@pytest.fixture(scope="module")
def nbco(engine_lib):
    if not os.path.exists(NBCO):
        subprocess.check_call(["make", "-C", os.path.dirname(NBCO), "-s", "nbco"])
    return NBCO


def test_help_mentions_the_energy_flag(nbco):
    r = subprocess.run([nbco, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "-energy" in r.stdout and "energy.txt" in r.stdout
