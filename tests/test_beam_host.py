"""The numpy reference of the beam diagnostics (tests/beam_numpy.py) against closed forms, and the library's host-only derivation
nbco_moments_derive against the reference.  No GPU."""
import ctypes
import math

import numpy as np

import beam_numpy as BN
import fmm2d_numpy as F

N_BEAM = 65536


def lattice_2d():
    """the full product lattice x in -2..2, y in -1..1, vx in {-1, 1}, vy in {-3, 0, 3}: 90 particles, every odd moment 0 and
    every even one a product of the axes' own"""
    g = np.array(np.meshgrid([-2, -1, 0, 1, 2], [-1, 0, 1], [-1, 1], [-3, 0, 3], indexing="ij"), dtype=np.float64).reshape(4, -1).T
    return np.stack([g[:, :2], g[:, 2:]])


def test_symmetric_lattice_has_the_moments_known_in_closed_form():
    m = BN.moments(lattice_2d(), 2)
    assert m["n"] == 90
    assert np.array_equal(m["mean"], np.zeros(6))
    assert m["min"][:4].tolist() == [-2, -1, -1, -3] and m["max"][:4].tolist() == [2, 1, 1, 3]
    want = np.zeros((6, 6))
    want[0, 0], want[1, 1], want[2, 2], want[3, 3] = 2.0, 2.0 / 3.0, 1.0, 6.0
    assert np.allclose(m["cov"], want, rtol=0, atol=1e-15)
    assert np.allclose(m["m4"][0], [6.8, 0, 2.0, 0, 1.0], rtol=0, atol=1e-14)
    assert np.allclose(m["m4"][1], [2.0 / 3.0, 0, 4.0, 0, 54.0], rtol=0, atol=1e-14)
    assert np.array_equal(m["m4"][2], np.zeros(5))
    assert np.allclose(m["emit"], [math.sqrt(2.0), 2.0, 0.0], rtol=1e-15)
    assert np.allclose(m["halo_q"], [6.8 / 4.0 - 2.0, (2.0 / 3.0) / (4.0 / 9.0) - 2.0, 0.0], rtol=1e-14)
    i4 = [6.8 * 1.0 + 3.0 * 4.0, (2.0 / 3.0) * 54.0 + 3.0 * 16.0]
    assert np.allclose(m["halo"], [math.sqrt(3 * i4[0]) / 4.0 - 2.0, math.sqrt(3 * i4[1]) / 8.0 - 2.0, 0.0], rtol=1e-14)


def test_kv_beam_has_halo_0_and_gaussian_beam_has_halo_1(engine_lib):
    """init2d at n = 65 536.  The sampling error of a kurtosis ratio at that n is 0.004 - 0.01: 0.05 is more than five standard
    errors and far from the 1.0 that separates the two distributions."""
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _om0 = F.kv_params()
    kv = BN.moments(init2d(N_BEAM, "kv", A, om), 2)
    assert np.abs(kv["halo_q"][:2]).max() < 0.05, kv["halo_q"]
    assert np.abs(kv["halo"][:2]).max() < 0.05, kv["halo"]
    ga = BN.moments(init2d(N_BEAM, "ga", [0.5 * A[0], 0.5 * A[1]], [0.5 * A[0] * om[0], 0.5 * A[1] * om[1]]), 2)
    assert np.abs(ga["halo_q"][:2] - 1.0).max() < 0.05, ga["halo_q"]
    assert np.abs(ga["halo"][:2] - 1.0).max() < 0.05, ga["halo"]
    # both are centred with exactly the requested rms sizes (main.cu:120-170)
    for m in (kv, ga):
        assert np.abs(m["mean"]).max() < 1e-15
        assert np.allclose(np.sqrt(np.diag(m["cov"])[:2]), [0.5 * A[0], 0.5 * A[1]], rtol=1e-12)


def test_zero_conventions_give_zeros_not_nan():
    one = np.array([[[0.3, -0.2, 0.1]], [[1.0, 2.0, 3.0]]])
    coincident = np.repeat(one, 7, axis=1)
    flat = np.random.default_rng(3).normal(size=(2, 50, 3))
    flat[0, :, 2] = 0.1        # z constant
    flat[1, :, 1] = 0.0        # vy exactly 0
    for st in (one, coincident, flat):
        m = BN.moments(st, 3)
        for k in ("mean", "cov", "m4", "emit", "halo_q", "halo"):
            assert np.isfinite(m[k]).all(), k
    for st in (one, coincident):
        m = BN.moments(st, 3)
        assert not m["cov"].any() and not m["m4"].any() and not m["emit"].any() and not m["halo_q"].any() and not m["halo"].any()
    m = BN.moments(flat, 3)
    assert not m["cov"][2].any() and not m["cov"][4].any()
    assert m["emit"][0] > 0 and m["emit"][1] == 0 and m["emit"][2] == 0
    assert m["halo"][1] == 0 and m["halo"][2] == 0 and m["halo_q"][2] == 0 and m["halo_q"][1] != 0


def test_bin_rule_agrees_with_numpy_histograms():
    """data with no point on an edge: np.histogram and np.histogram2d over the same window count what the bin rule counts"""
    rng = np.random.default_rng(11)
    n = 20000
    st = rng.uniform(-1.5, 1.5, size=(2, n, 3))
    q = BN.phase_space(st, 3)
    for coord, bins, lo, hi in ((0, 1, -1.0, 1.0), (1, 7, -1.0, 0.5), (5, 1000, -0.3, 1.4), (3, 64, -2.0, 2.0)):
        got = BN.hist(st, 3, [(coord, bins, lo, hi)])
        want, _ = np.histogram(q[:, BN.coord_index(coord, 3)], bins=bins, range=(lo, hi))
        assert np.array_equal(got[:bins], want)
        assert got[bins] == n - want.sum() and got.sum() == n
    for (c0, b0, lo0, hi0), (c1, b1, lo1, hi1) in (((0, 3, -1.0, 1.0), (1, 5, -1.0, 1.0)), ((4, 64, -1.2, 0.9), (1, 33, -0.1, 2.0))):
        got = BN.hist(st, 3, [(c0, b0, lo0, hi0), (c1, b1, lo1, hi1)])
        want, _, _ = np.histogram2d(q[:, BN.coord_index(c0, 3)], q[:, BN.coord_index(c1, 3)], bins=(b0, b1), range=((lo0, hi0), (lo1, hi1)))
        assert np.array_equal(got[:-1].reshape(b0, b1), want.astype(np.int64))
        assert got.sum() == n


def test_bin_rule_on_the_edges():
    """lo is inside, hi is outside, an interior edge belongs to the bin above it, a NaN is outside"""
    x = np.array([-4.0, -3.0, 0.0, 3.0, 3.999, 4.0, -4.001, np.nan])
    st = np.zeros((2, len(x), 2))
    st[0, :, 0] = x
    got = BN.hist(st, 2, [(0, 8, -4.0, 4.0)])
    assert got.tolist() == [1, 1, 0, 0, 1, 0, 0, 2, 3]
    assert BN.coord_index(2, 2) is None and BN.coord_index(5, 2) is None and BN.coord_index(4, 2) == 3


def test_library_derivation_is_the_reference_formula(engine_lib):
    """nbco_moments_derive (host only): emit, halo_q, halo of a structure whose cov and m4 come from the reference; relative 1e-13
    allows for a fused multiply-add in the host compiler's I2 and I4 and nothing else"""
    from coulomb_oscillators_amd.engine import Moments, _load
    assert ctypes.sizeof(Moments) == 8 + 8 + 8 * (18 + 36 + 15 + 9)
    lib = _load()
    rng = np.random.default_rng(5)
    for dim in (2, 3):
        q = rng.normal(size=(3000, dim)) * np.arange(1, dim + 1)
        st = np.stack([q, 0.6 * q + rng.normal(size=q.shape)])
        st[1, :, dim - 1] = 0.25          # one flat velocity axis: that plane's emit and halo are 0, its halo_q is not
        ref = BN.moments(st, dim)
        m = Moments()
        m.n, m.dim = 3000, dim
        for a in range(6):
            for b in range(6):
                m.cov[a][b] = ref["cov"][a, b]
        for k in range(3):
            for j in range(5):
                m.m4[k][j] = ref["m4"][k, j]
        m.emit[0] = m.halo[2] = float("nan")      # overwritten
        assert lib.nbco_moments_derive(ctypes.byref(m)) == 0
        for name in ("emit", "halo_q", "halo"):
            got = np.array(getattr(m, name)[:])
            assert np.allclose(got, ref[name], rtol=1e-13, atol=0), (name, got, ref[name])
        assert m.emit[dim - 1] == 0 and m.halo[dim - 1] == 0 and m.halo_q[dim - 1] != 0
    m = Moments()
    m.dim = 4
    assert lib.nbco_moments_derive(ctypes.byref(m)) != 0 and lib.nbco_moments_derive(None) != 0


def test_raw_power_sums_lose_the_fourth_moment_of_a_beam_off_the_origin():
    """why the device takes two passes: for a beam of size 1 centred at 1000 (fp32 coordinates) the fourth central moment formed from
    sums of raw powers -- each sum exactly rounded here -- misses the central form by 1e-4 to 1e-3, millions of times the bound the GPU
    test sets for the central sums"""
    rng = np.random.default_rng(2)
    x = (1000.0 + rng.normal(size=20000)).astype(np.float32).astype(np.float64)
    mu = BN.fmean(x)
    central = BN.fmean((x - mu) ** 4)
    raw = BN.fmean(x ** 4) - 4.0 * mu * BN.fmean(x ** 3) + 6.0 * mu * mu * BN.fmean(x ** 2) - 3.0 * mu ** 4
    assert 2.0 < central < 4.0
    assert abs(raw - central) > 1e-6 * central, (raw, central)
