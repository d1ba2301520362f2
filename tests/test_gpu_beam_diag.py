"""GPU tests of the beam diagnostics: nbco_beam_moments / nbco_2d_beam_moments (Engine.beam_moments, beam_moments_2d) and nbco_hist /
nbco_2d_hist (Engine.hist, hist_2d) against the fp64 numpy reference tests/beam_numpy.py, at every size where the launch shape
changes, on exact, off-origin and degenerate data, and the calls' contract: repeatable, read-only, refusing before any launch, and
leaving a kd-tree evaluation's diagnostics bit for bit as they were.

The bound on a sum field (mean, cov, m4) is 1e-10 x (mean absolute value of that sum's terms).  It is derived, not measured: any
summation order of n <= 262 145 fp64 terms errs by at most n 2^-53 = 2.9e-11 of the sum of absolute terms; the roundings of the
terms and the effect of the mean's own error on the fourth-order sums are a few times that; a dropped lane, tail or block errs at
1 / n >= 4e-6."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import beam_numpy as BN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coulomb_oscillators_amd", "csrc")
ERR_ARG = 2
DIMS = [3, 2]
DTYPE = {3: np.float32, 2: np.float64}
X, Y, Z, VX, VY, VZ = range(6)
PAIRS = [(X, Y), (X, VX), (VY, Y)]
SIGMA = np.array([1.0, 0.3, 2.5])
GARBAGE = -7777


def _const(fname, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read()).group(1))


ONE_PASS = _const("k_reduce.hip", "kBlock") * _const("k_reduce.hip", "kMaxBlocks")   # particles one grid pass of the reductions covers
LDS_BINS = _const("beam_diag_kernels.hpp", "kHistLdsBins")                            # the histogram's LDS budget
PER_BLOCK = _const("beam_diag_kernels.hpp", "kHistPerBlock")                          # particles per workgroup of its LDS form
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, ONE_PASS + 1]
HIST_SIZES = SIZES[:-1] + [PER_BLOCK, PER_BLOCK + 1, ONE_PASS + 1]


@functools.lru_cache(maxsize=None)
def ball(dim, n=ONE_PASS + 1, seed=0, centre=0.0):
    """a correlated anisotropic ball [2, n, dim]: q = sigma o N(0, 1) about `centre`, p = 0.6 (q - centre) + sigma o N(0, 1) / 2
    (correlation 0.77: I2 is not a cancellation), rounded to the state's number format"""
    rng = np.random.default_rng([seed, dim, n])
    q = rng.normal(size=(n, dim)) * SIGMA[:dim]
    p = 0.6 * q + 0.5 * rng.normal(size=(n, dim)) * SIGMA[:dim]
    st = np.stack([q + centre, p]).astype(DTYPE[dim])
    st.setflags(write=False)
    return st


def head(st, n):
    return np.ascontiguousarray(st[:, :n])


@functools.lru_cache(maxsize=None)
def ball_reference(dim, n):
    return BN.moments(head(ball(dim), n), dim)


def dev(st):
    import torch
    return torch.from_numpy(np.ascontiguousarray(st).reshape(-1).copy()).cuda()


@pytest.fixture(scope="module")
def eng(engine_lib):
    import torch
    from coulomb_oscillators_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    e = Engine()
    yield e
    e.close()


def moments_fn(e, dim):
    return e.beam_moments if dim == 3 else e.beam_moments_2d


def hist_fn(e, dim):
    return e.hist if dim == 3 else e.hist_2d


def flat(m):
    """every field of a Moments structure as one float64 vector (compared as bytes)"""
    return np.concatenate([[m.n, m.dim]] + [np.array(getattr(m, k)).reshape(-1) for k in ("mean", "min", "max", "cov", "m4", "emit", "halo_q", "halo")])


def check_moments(m, ref, dim, what, fields=("mean", "cov", "m4")):
    assert m.n == ref["n"] and m.dim == dim, what
    assert np.array_equal(np.array(m.min), ref["min"]) and np.array_equal(np.array(m.max), ref["max"]), what
    worst = 0.0
    for k in fields:
        got, want, scale = np.array(getattr(m, k)), ref[k], ref["scale"][k]
        assert np.isfinite(got).all(), (what, k)
        err = np.abs(got - want)
        assert (err <= 1e-10 * scale).all(), (what, k, err.max(), scale[err > 1e-10 * scale])
        worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0)
    assert np.array_equal(np.array(m.cov), np.array(m.cov).T), what
    # the derived fields as functions of the RETURNED sums: a fused multiply-add in the host's compiler and nothing else
    der = BN.derived(np.array(m.cov), np.array(m.m4), dim)
    for k in ("emit", "halo_q", "halo"):
        assert np.allclose(np.array(getattr(m, k)), der[k], rtol=1e-13, atol=0), (what, k, np.array(getattr(m, k)), der[k])
    return worst


# ---- moments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_moments_at_every_launch_shape(eng, dim):
    worst = 0.0
    for n in SIZES:
        st = head(ball(dim), n)
        d = dev(st)
        m = moments_fn(eng, dim)(d, n)
        worst = max(worst, check_moments(m, ball_reference(dim, n), dim, (dim, n)))
        assert np.array_equal(d.cpu().numpy(), st.reshape(-1)), "the state was modified"
    print("dim %d: worst deviation of a sum from the reference, in units of the mean absolute term: %.2e" % (dim, worst))


@pytest.mark.parametrize("dim", DIMS)
def test_moments_of_integer_pairs_are_exact(eng, dim):
    """n = 4096 small-integer coordinates in +-q pairs: the means are exactly 0 and every sum is an integer over a power of two, so
    cov and m4 equal the reference in every field"""
    rng = np.random.default_rng([1, dim])
    h = rng.integers(-8, 9, size=(2, 2048, dim))
    st = np.concatenate([h, -h], axis=1).astype(DTYPE[dim])
    m = moments_fn(eng, dim)(dev(st), 4096)
    ref = BN.moments(st, dim)
    assert not np.array(m.mean).any() and not ref["mean"].any()
    for k in ("min", "max", "cov", "m4"):
        assert np.array_equal(np.array(getattr(m, k)), ref[k]), k
    check_moments(m, ref, dim, "integer pairs")


@pytest.mark.parametrize("dim", DIMS)
def test_moments_of_a_beam_off_the_origin(eng, dim):
    """centre 1000, sigma of order 1 (fp32 in 3-D): the central form keeps the fourth moments within the bound; sums of raw powers
    lose them to cancellation at about 1e-4"""
    n = 20000
    st = ball(dim, n, 2, 1000.0)
    m = moments_fn(eng, dim)(dev(st), n)
    ref = BN.moments(st, dim)
    assert abs(ref["mean"][0] - 1000.0) < 0.1 and 0.5 < ref["m4"][0, 0] < 10.0
    check_moments(m, ref, dim, "off-origin")


@pytest.mark.parametrize("dim", DIMS)
def test_moments_of_degenerate_shapes(eng, dim):
    """all particles coincident; one axis constant; all velocities exactly 0: cov is exactly 0 where it must be, the derived fields
    are 0 there, nothing is NaN.  (0.3 and 0.7 are not sums of few powers of two: n copies of them do not add up to n times them)"""
    n = 1000
    base = np.array(ball(dim, n, 3))
    coincident = np.empty_like(base)
    coincident[0], coincident[1] = 0.3, -0.7
    flat_axis = base.copy()
    flat_axis[0, :, 1] = 0.3
    cold = base.copy()
    cold[1] = 0.0
    for name, st in (("coincident", coincident), ("flat axis", flat_axis), ("cold", cold)):
        m = moments_fn(eng, dim)(dev(st), n)
        ref = BN.moments(st, dim)
        assert np.isfinite(flat(m)).all(), name
        check_moments(m, ref, dim, name)
        cov, zero = np.array(m.cov), ref["cov"] == 0
        assert (cov[zero] == 0).all(), name
        for k in ("emit", "halo_q", "halo"):
            assert (np.array(getattr(m, k))[ref[k] == 0] == 0).all(), (name, k)
        if name == "coincident":
            assert not cov.any() and not np.array(m.m4).any() and not np.array(m.emit).any() and not np.array(m.halo_q).any() and not np.array(m.halo).any()
            assert np.array_equal(np.array(m.mean), ref["mean"]) and np.array_equal(np.array(m.min), np.array(m.max))
        if name == "flat axis":
            assert not cov[1].any() and m.emit[1] == 0 and m.halo[1] == 0 and m.halo_q[1] == 0 and m.emit[0] > 0 and m.mean[1] == ref["mean"][1]
        if name == "cold":
            assert not cov[dim:].any() and not np.array(m.emit).any() and not np.array(m.halo).any() and (np.array(m.halo_q)[:dim] != 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_moments_contract(eng, dim):
    """a second call returns identical bytes; the state is unchanged byte for byte; a non-default stream and sync = 0 work; the
    refusals return NBCO_ERR_ARG and leave *out_host as it was"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, Moments
    n = 5000
    st = head(ball(dim), n)
    d = dev(st)
    first = flat(moments_fn(eng, dim)(d, n))
    assert flat(moments_fn(eng, dim)(d, n)).tobytes() == first.tobytes()
    assert np.array_equal(d.cpu().numpy(), st.reshape(-1))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = Engine(sync=0)
        try:
            assert flat(moments_fn(other, dim)(d, n)).tobytes() == first.tobytes()
        finally:
            other.close()
    fn = eng.lib.nbco_beam_moments if dim == 3 else eng.lib.nbco_2d_beam_moments
    out = Moments()
    ctypes.memset(ctypes.byref(out), 0x5a, ctypes.sizeof(out))
    before = bytes(out)
    ptr = ctypes.c_void_p(d.data_ptr())
    for args in ((None, n), (ptr, 0), (ptr, -3)):
        assert fn(eng.ctx, args[0], args[1], ctypes.byref(out)) == ERR_ARG, args
        assert bytes(out) == before, args
    assert fn(eng.ctx, ptr, n, None) == ERR_ARG
    with pytest.raises(EngineError) as ei:
        moments_fn(eng, dim)(d, 0)
    assert ei.value.status == ERR_ARG
    assert flat(moments_fn(eng, dim)(d, n)).tobytes() == first.tobytes()


def test_diagnostics_leave_a_kd_evaluation_as_it_was(oracle32):
    """a kd evaluation followed by beam_moments and hist, then energy_kd, energy_fmm and probe_kd: the bits they return without the
    diagnostics in between; the same after 2-D calls on the same context, and the diagnostics equal a fresh context's"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    n, p = 3000, 4
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    e = Engine(fmm_order=p, unsort=1)
    fresh = Engine()
    try:
        d, prm = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda()
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        t = torch.from_numpy(np.ascontiguousarray(buf[0][:300] * np.float32(1.3))).cuda()

        def look():
            phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            a = torch.full((300, 3), float("nan"), dtype=torch.float64, device="cuda")
            psi = torch.full((300,), float("nan"), dtype=torch.float64, device="cuda")
            ek, ef = e.energy_kd(d, n, prm, phi), e.energy_fmm(d, n, prm)
            e.probe_kd(t, 300, prm, a, psi)
            got = np.concatenate([np.asarray(ek), np.asarray(ef), phi.cpu().numpy(), a.cpu().numpy().reshape(-1), psi.cpu().numpy()])
            assert np.isfinite(got).all()
            return got.tobytes()
        axes = [(X, 64, -0.004, 0.005), (VX, 64, -0.005, 0.004)]
        big = [(X, 512, -0.004, 0.005), (Y, 512, -0.002, 0.002)]
        before = look()
        m3 = flat(e.beam_moments(d, n))
        h3, h3big = e.hist(d, n, axes).cpu().numpy(), e.hist(d, n, big).cpu().numpy()
        assert look() == before
        st2 = head(ball(2), 2500)
        d2 = dev(st2)
        m2 = flat(e.beam_moments_2d(d2, 2500))
        h2 = e.hist_2d(d2, 2500, [(X, 3, -1.0, 2.0), (VY, 5, -0.2, 0.3)]).cpu().numpy()
        assert look() == before
        assert flat(e.beam_moments(d, n)).tobytes() == m3.tobytes() == flat(fresh.beam_moments(d, n)).tobytes()
        assert flat(fresh.beam_moments_2d(d2, 2500)).tobytes() == m2.tobytes()
        assert np.array_equal(fresh.hist(d, n, axes).cpu().numpy(), h3) and np.array_equal(fresh.hist(d, n, big).cpu().numpy(), h3big)
        assert np.array_equal(fresh.hist_2d(d2, 2500, [(X, 3, -1.0, 2.0), (VY, 5, -0.2, 0.3)]).cpu().numpy(), h2)
        assert np.array_equal(h3, BN.hist(buf[:2], 3, axes)) and np.array_equal(h3big, BN.hist(buf[:2], 3, big))
        check_moments(e.beam_moments(d, n), BN.moments(buf[:2], 3), 3, "initial state")
    finally:
        e.close()
        fresh.close()


# ---- density maps ------------------------------------------------------------------------------------------------------------------
def window(st, dim, coord, k=0):
    """a window that cuts the beam off-centre: [mean - 1.3 std, mean + 1.7 std) of the coordinate (k shifts it a little)"""
    q = BN.phase_space(st, dim)[:, BN.coord_index(coord, dim)]
    mu, sd = float(q.mean()), float(q.std()) or 1.0
    return mu - (1.3 + 0.1 * k) * sd, mu + (1.7 - 0.1 * k) * sd


@functools.lru_cache(maxsize=None)
def ball_window(dim, coord, k=0):
    return window(ball(dim), dim, coord, k)


def check_hist(e, dim, st, d, axes, what=None):
    """one call into a buffer pre-filled with garbage: the counts are the reference's, integer for integer, and add up to n"""
    import torch
    n = st.shape[1]
    B = int(np.prod([a[1] for a in axes]))
    counts = torch.full((B + 1,), GARBAGE, dtype=torch.int64, device="cuda")
    got = hist_fn(e, dim)(d, n, axes, counts)
    assert got is counts
    h = counts.cpu().numpy()
    want = BN.hist(st, dim, axes)
    assert h.sum() == n, (what, axes)
    assert np.array_equal(h, want), (what, axes, np.flatnonzero(h != want)[:8])
    return h


@pytest.mark.parametrize("dim", DIMS)
def test_hist_at_every_launch_shape(eng, dim):
    """sizes where the launch shape changes x profiles of 1, 2, 64, 1000 bins x maps of 1 x 1, 3 x 5, 64 x 64 and 512 x 512 bins (above
    the LDS budget) over the pairs (X, Y), (X, VX), (VY, Y); the budget itself from both sides"""
    coords = [X, Y, VX, VY] if dim == 2 else [X, Y, Z, VX, VY, VZ]
    full = ball(dim)
    assert 64 * 64 <= LDS_BINS < 512 * 512
    r = int(round(LDS_BINS ** 0.5))
    assert r * r == LDS_BINS
    k = 0
    for n in HIST_SIZES:
        st = head(full, n)
        d = dev(st)
        for bins in (1, 2, 64, 1000):
            c = coords[k % len(coords)]
            k += 1
            check_hist(eng, dim, st, d, [(c, bins) + ball_window(dim, c, k % 3)], n)
        for b0, b1 in ((1, 1), (3, 5), (64, 64), (512, 512)):
            for c0, c1 in PAIRS:
                check_hist(eng, dim, st, d, [(c0, b0) + ball_window(dim, c0), (c1, b1) + ball_window(dim, c1, 1)], n)
        if n in (1000, ONE_PASS + 1):
            for axes in ([(X, LDS_BINS) + ball_window(dim, X)], [(X, LDS_BINS + 1) + ball_window(dim, X)],
                         [(VX, r) + ball_window(dim, VX), (Y, r) + ball_window(dim, Y)],
                         [(VX, r) + ball_window(dim, VX), (Y, r + 1) + ball_window(dim, Y)]):
                check_hist(eng, dim, st, d, axes, n)
        assert np.array_equal(d.cpu().numpy(), st.reshape(-1)), "the state was modified"


@pytest.mark.parametrize("dim", DIMS)
def test_hist_edges_and_corner_cases(eng, dim):
    import torch
    # integer data with lo = -4, hi = 4, bins = 8: values sit exactly on lo (inside), on hi (outside) and on interior edges
    rng = np.random.default_rng([4, dim])
    n = 3001
    st = rng.integers(-5, 6, size=(2, n, dim)).astype(DTYPE[dim])
    d = dev(st)
    h = check_hist(eng, dim, st, d, [(X, 8, -4.0, 4.0)])
    x = st[0, :, 0]
    assert h.tolist() == [int((x == v).sum()) for v in range(-4, 4)] + [int(((x < -4) | (x >= 4)).sum())]
    check_hist(eng, dim, st, d, [(VY, 8, -4.0, 4.0), (Y, 8, -4.0, 4.0)])
    check_hist(eng, dim, st, d, [(X, 3, -4.0, 4.0), (VX, 1000, -4.0, 4.0)])          # bin widths that are no powers of two
    # 100 000 particles in one bin
    n = 100000
    st = np.empty((2, n, dim), dtype=DTYPE[dim])
    st[0], st[1] = 0.25, -0.5
    d = dev(st)
    for axes in ([(X, 64, -1.0, 1.0), (VX, 64, -1.0, 1.0)], [(X, 1000, -1.0, 1.0)], [(X, 512, -1.0, 1.0), (VY, 512, -1.0, 1.0)]):
        h = check_hist(eng, dim, st, d, axes)
        assert h.max() == n and np.count_nonzero(h) == 1 and h[-1] == 0
    # a window that misses the beam
    for axes in ([(X, 64, 5.0, 6.0)], [(X, 64, -1.0, 1.0), (VX, 64, 0.0, 1.0)], [(X, 600, -1.0, 1.0), (VX, 600, -2.0, -0.5000001)]):
        h = check_hist(eng, dim, st, d, axes)
        assert h[-1] == n and not h[:-1].any()
    # one NaN coordinate is outside on its axis and nowhere else
    st = np.array(head(ball(dim), 777))
    st[0, 5, 0] = np.nan
    d = dev(st)
    wide = (-100.0, 100.0)
    assert check_hist(eng, dim, st, d, [(X, 16) + wide])[-1] == 1
    assert check_hist(eng, dim, st, d, [(Y, 16) + wide, (X, 16) + wide])[-1] == 1
    assert check_hist(eng, dim, st, d, [(Y, 16) + wide, (VX, 16) + wide])[-1] == 0
    # the largest axis and the largest grid are accepted
    st = head(ball(dim), 1000)
    d = dev(st)
    check_hist(eng, dim, st, d, [(X, 65536) + window(st, dim, X)])
    if dim == 3:
        check_hist(eng, dim, st, d, [(X, 4096) + window(st, dim, X), (VX, 4096) + window(st, dim, VX)])
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dim", DIMS)
def test_hist_contract(eng, dim):
    """a second call returns equal counts; a non-default stream and sync = 0 work; counts are allocated when not given; every refusal
    returns NBCO_ERR_ARG before any launch and leaves counts_dev untouched"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, HistAxis
    n = 5000
    st = head(ball(dim), n)
    d = dev(st)
    ax1 = [(VX, 100) + window(st, dim, VX)]
    ax2 = [(X, 48) + window(st, dim, X), (VY, 52) + window(st, dim, VY)]
    for axes in (ax1, ax2):
        first = check_hist(eng, dim, st, d, axes)
        assert np.array_equal(check_hist(eng, dim, st, d, axes), first)
        got = hist_fn(eng, dim)(d, n, axes)
        assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), first)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            other = Engine(sync=0)
            try:
                h = hist_fn(other, dim)(d, n, axes)
                other.sync()
                assert np.array_equal(h.cpu().numpy(), first)
            finally:
                other.close()
    assert np.array_equal(hist_fn(eng, dim)(d, n, ax1[0]).cpu().numpy(), BN.hist(st, dim, ax1))       # one tuple instead of a list

    fn = eng.lib.nbco_hist if dim == 3 else eng.lib.nbco_2d_hist
    counts = torch.full((1 << 12,), GARBAGE, dtype=torch.int64, device="cuda")
    ptr, cptr = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(counts.data_ptr())

    def refused(buf, n_, axes, naxes, out, why):
        arr = (HistAxis * 3)(*[HistAxis(*a) for a in axes]) if axes is not None else None
        assert fn(eng.ctx, buf, n_, arr, naxes, out) == ERR_ARG, why
        assert bool((counts == GARBAGE).all()), why
    ok = (X, 8, -1.0, 1.0)
    nan, inf = float("nan"), float("inf")
    refused(None, n, [ok], 1, cptr, "NULL buf")
    refused(ptr, n, None, 1, cptr, "NULL axes")
    refused(ptr, n, [ok], 1, None, "NULL counts")
    refused(ptr, 0, [ok], 1, cptr, "n = 0")
    refused(ptr, -1, [ok], 1, cptr, "n < 0")
    refused(ptr, n, [ok], 0, cptr, "no axis")
    refused(ptr, n, [ok, ok, ok], 3, cptr, "three axes")
    refused(ptr, n, [(-1, 8, -1.0, 1.0)], 1, cptr, "coordinate -1")
    refused(ptr, n, [(6, 8, -1.0, 1.0)], 1, cptr, "coordinate 6")
    refused(ptr, n, [ok, (7, 8, -1.0, 1.0)], 2, cptr, "coordinate 7 on the second axis")
    if dim == 2:
        refused(ptr, n, [(Z, 8, -1.0, 1.0)], 1, cptr, "Z in 2-D")
        refused(ptr, n, [ok, (VZ, 8, -1.0, 1.0)], 2, cptr, "VZ in 2-D")
    refused(ptr, n, [(X, 0, -1.0, 1.0)], 1, cptr, "bins = 0")
    refused(ptr, n, [(X, -4, -1.0, 1.0)], 1, cptr, "bins < 0")
    refused(ptr, n, [(X, 65537, -1.0, 1.0)], 1, cptr, "bins > 65536")
    refused(ptr, n, [(X, 4097, -1.0, 1.0), (Y, 4096, -1.0, 1.0)], 2, cptr, "B > 2^24")
    refused(ptr, n, [(X, 65536, -1.0, 1.0), (Y, 65536, -1.0, 1.0)], 2, cptr, "B = 2^32")
    refused(ptr, n, [(X, 8, nan, 1.0)], 1, cptr, "lo NaN")
    refused(ptr, n, [(X, 8, -1.0, nan)], 1, cptr, "hi NaN")
    refused(ptr, n, [(X, 8, -inf, 1.0)], 1, cptr, "lo -inf")
    refused(ptr, n, [ok, (Y, 8, -1.0, inf)], 2, cptr, "hi inf")
    refused(ptr, n, [(X, 8, 1.0, 1.0)], 1, cptr, "lo = hi")
    refused(ptr, n, [ok, (Y, 8, 1.0, -1.0)], 2, cptr, "lo > hi")
    with pytest.raises(EngineError) as ei:
        hist_fn(eng, dim)(d, n, [(X, 0, -1.0, 1.0)])
    assert ei.value.status == ERR_ARG
    check_hist(eng, dim, st, d, ax2)                                                                  # and a good call afterwards
