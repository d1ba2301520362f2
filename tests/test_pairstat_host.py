"""The fp64 reference of the pair statistics (tests/pairstat_numpy.py) against a plain double loop and against exact integer
arithmetic, and the source rule its kernels depend on.  No GPU."""
import os

import numpy as np
import pytest

import pairstat_numpy as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coulomb_oscillators_amd", "csrc")


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_vectorised_reference_is_the_double_loop(n, dim):
    """a ball of sigma 1e-3; the windows hold some, most and all of the pairs, with one bin and with many"""
    rng = np.random.default_rng(100 * n + dim)
    pos = (rng.standard_normal((n, dim)) * 1e-3).astype(np.float32 if dim == 3 else np.float64)
    for rmax in (5e-4, 2e-3, 1.0):
        for bins in (1, 7, 64):
            c, m = PN.pair_hist(pos, bins, rmax, chunk=16)
            c0, m0 = PN.pair_hist_loops(pos, bins, rmax)
            assert np.array_equal(c, c0), (rmax, bins)
            assert m.tobytes() == m0.tobytes(), (rmax, bins)
            assert c.sum() == n * (n - 1) // 2
    if n == 65:
        c, m = PN.pair_hist(pos, 64, 5e-4)
        assert 0 < c[:64].sum() < c.sum() and np.isinf(m).any() and np.isfinite(m).any()   # a sparse window


def test_integer_lattice_against_integer_arithmetic():
    pos, want = PN.lattice()
    n = len(pos)
    c, m = PN.pair_hist(pos, PN.LATTICE_BINS, PN.LATTICE_RMAX)
    assert np.array_equal(c, want) and c.sum() == n * (n - 1) // 2
    # pairs at exactly r = 0.5 k sit in bin k: on this lattice r = 1, 2, 3 (k = 2, 4, 6) along an axis, and nothing else reaches
    # those bins' lower edges from below
    axis = {1: 3 * 4 * 25, 2: 3 * 3 * 25, 3: 3 * 2 * 25}   # pairs at distance exactly k along one axis
    assert c[2] >= axis[1] and c[4] >= axis[2] and c[6] >= axis[3]
    one = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [4, 0, 0]], dtype=np.float32)
    c1, _ = PN.pair_hist(one[[0, 1]], 8, 4.0)
    c2, _ = PN.pair_hist(one[[0, 2]], 8, 4.0)
    c3, _ = PN.pair_hist(one[[0, 3]], 8, 4.0)
    c4, m4 = PN.pair_hist(one[[0, 4]], 8, 4.0)
    assert c1[2] == 1 and c2[4] == 1 and c3[6] == 1
    assert c4[8] == 1 and c4[:8].sum() == 0 and np.isinf(m4).all()   # exactly r = 4 is outside
    assert (m == 1.0).all()


def test_coincident_particles_fill_bin_zero():
    pos = np.full((40, 3), 0.25, dtype=np.float32)
    c, m = PN.pair_hist(pos, 16, 1e-3)
    assert c[0] == 40 * 39 // 2 and c[1:].sum() == 0
    assert (m == 0.0).all()
    pos2 = np.full((40, 2), -3.0)
    c, m = PN.pair_hist(pos2, 1, 1e-150)
    assert c[0] == 40 * 39 // 2 and (m == 0.0).all()
    c, m = PN.pair_hist(pos2, 1, 1e-200)            # rmax * rmax underflows to 0: r2 = 0 is not below it
    assert c[1] == 40 * 39 // 2 and np.isinf(m).all()


def test_a_nan_coordinate_is_outside():
    rng = np.random.default_rng(3)
    pos = (rng.standard_normal((30, 3)) * 1e-3).astype(np.float32)
    c0, m0 = PN.pair_hist(pos, 8, 1.0)
    bad = pos.copy()
    bad[11, 1] = np.nan
    c, m = PN.pair_hist(bad, 8, 1.0)
    assert c[8] == 29 and c.sum() == 30 * 29 // 2 and np.isinf(m[11])
    keep = np.arange(30) != 11
    c_rest, m_rest = PN.pair_hist(pos[keep], 8, 1.0)
    assert np.array_equal(c[:8], c_rest[:8]) and m[keep].tobytes() == m_rest.tobytes()


def _state_at_definitions(path, names):
    """tests/test_source_rules.py's reading of a source file: the `fp contract` state in force where a function is DEFINED"""
    import re
    state, out = "default", {}
    for line in open(path):
        m = re.search(r"#pragma clang fp contract\((\w+)\)", line)
        if m:
            state = m.group(1)
        for n in names:
            if n not in out and re.search(r"\b%s\s*\(" % re.escape(n), line) and ("__device__" in line or "__global__" in line):
                out[n] = state
    return out


def test_pair_rule_is_compiled_without_contraction():
    """the library is built with -ffp-contract=on: a contracted dx dx + dy dy moves a pair across a bin edge once in millions"""
    names = ["pair_r2", "pair_lower2", "pair_bin"]
    got = _state_at_definitions(os.path.join(CSRC, "pair_stat_kernels.hpp"), names)
    for n in names:
        assert got.get(n) == "off", (n, got.get(n))
    # and both translation units take the section in
    for unit in ("k_reduce.hip", "k_fmm_kd.hip"):
        assert '#include "pair_stat_kernels.hpp"' in open(os.path.join(CSRC, unit)).read(), unit
