"""The fp64 reference of the slice diagnostics (tests/slice_numpy.py) held to closed forms; needs no GPU."""
import itertools
import math

import numpy as np
import pytest

import beam_numpy as BN
import slice_numpy as SN

X, Y, Z, VX, VY, VZ = range(6)
SIGMA = np.array([1.0, 0.3, 2.5])


def ball(dim, n, seed=0):
    rng = np.random.default_rng([seed, dim, n])
    q = rng.normal(size=(n, dim)) * SIGMA[:dim]
    p = 0.6 * q + 0.5 * rng.normal(size=(n, dim)) * SIGMA[:dim]
    return np.stack([q, p])


@pytest.mark.parametrize("dim", [3, 2])
def test_slices_of_a_symmetric_lattice_have_its_transverse_moments(dim):
    """every point of {-2 .. 2}^(2 dim), shuffled, sliced along x into 5 slices: x is flat in a slice, every other coordinate has
    mean 0, <d^2> = 2, <d^4> = 6.8, <d^2 e^2> = 4 and no odd moment; emit = 2, halo_q = 6.8 / 4 - 2, halo = sqrt(3 I4) / 8 - 2
    with I4 = 6.8^2 + 3 * 4^2"""
    pts = np.array(list(itertools.product(range(-2, 3), repeat=2 * dim)), dtype=np.float64)
    pts = np.random.default_rng(1).permutation(pts)
    st = np.stack([pts[:, :dim], pts[:, dim:]])
    recs, outside = SN.slice_moments(st, dim, (X, 5, -2.5, 2.5))
    assert outside == 0 and len(recs) == 5
    for s, r in enumerate(recs):
        assert r["n"] == 5 ** (2 * dim - 1) and r["dim"] == dim
        mean = np.zeros(6)
        mean[0] = s - 2
        cov = np.zeros((6, 6))
        cov[1:2 * dim, 1:2 * dim] = 2.0 * np.eye(2 * dim - 1)
        m4 = np.zeros((3, 5))
        m4[1:dim] = [6.8, 0, 4, 0, 6.8]
        m4[0, 4] = 6.8   # the plane (x, vx): x is flat, vx is not
        assert np.array_equal(r["mean"], mean) and r["min"][0] == r["max"][0] == s - 2
        assert np.allclose(r["cov"], cov, rtol=1e-15, atol=0) and np.allclose(r["m4"], m4, rtol=1e-15, atol=0)
        halo = math.sqrt(3 * (6.8 ** 2 + 3 * 16)) / 8 - 2
        assert np.allclose(r["emit"][:dim], [0] + [2] * (dim - 1), rtol=1e-15, atol=0)
        assert np.allclose(r["halo_q"][:dim], [0] + [6.8 / 4 - 2] * (dim - 1), rtol=1e-14, atol=0)
        assert np.allclose(r["halo"][:dim], [0] + [halo] * (dim - 1), rtol=1e-14, atol=0)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("coord,bins", [(X, 16), (VY, 7), (Y, 1)])
def test_slices_recombine_to_the_moments_of_the_window(dim, coord, bins):
    """the law of total covariance: N = sum n_s, m = sum n_s m_s / N, cov = sum n_s (cov_s + (m_s - m)(m_s - m)^T) / N are the
    moments of the particles inside the window, to 1e-12 relative"""
    n = 5000
    st = ball(dim, n)
    q = BN.phase_space(st, dim)[:, BN.coord_index(coord, dim)]
    axis = (coord, bins, float(q.mean() - 1.3 * q.std()), float(q.mean() + 1.7 * q.std()))
    recs, outside = SN.slice_moments(st, dim, axis)
    inside, _ = BN.bin_of(q, *axis[1:])
    want = BN.moments(st[:, inside], dim)
    N = sum(r["n"] for r in recs)
    assert N == want["n"] == n - outside and 0 < outside < n
    Q = 2 * dim
    mean = np.array([math.fsum(r["n"] * r["mean"][a] for r in recs) / N for a in range(Q)])
    assert (np.abs(mean - want["mean"][:Q]) <= 1e-12 * np.abs(want["mean"][:Q])).all()
    for a in range(Q):
        for b in range(Q):
            c = math.fsum(r["n"] * (r["cov"][a, b] + (r["mean"][a] - mean[a]) * (r["mean"][b] - mean[b])) for r in recs) / N
            assert abs(c - want["cov"][a, b]) <= 1e-12 * abs(want["cov"][a, b]), (a, b)
    assert all(min(r["min"][a] for r in recs if r["n"]) == want["min"][a] and max(r["max"][a] for r in recs if r["n"]) == want["max"][a] for a in range(Q))


@pytest.mark.parametrize("dim", [3, 2])
def test_slice_counts_are_the_histogram(dim):
    """n per slice and n_outside are beam_numpy.hist of the same axis, also with empty slices, a NaN and values on the edges"""
    n = 3001
    st = np.random.default_rng([4, dim]).integers(-5, 6, size=(2, n, dim)).astype(np.float64)
    st[0, 17, 0] = np.nan
    for axis in ((X, 8, -4.0, 4.0), (X, 1000, -4.0, 4.0), (VY, 3, -4.0, 4.0), (Y, 65536, -7.0, 9.0), (X, 4, 20.0, 30.0)):
        recs, outside = SN.slice_moments(st, dim, axis)
        h = BN.hist(st, dim, [axis])
        assert [r["n"] for r in recs] == h[:-1].tolist() and outside == h[-1]
        for r in recs:
            if r["n"] == 0:
                assert r["dim"] == dim and not any(np.asarray(r[k]).any() for k in ("mean", "min", "max", "cov", "m4", "emit", "halo_q", "halo"))
