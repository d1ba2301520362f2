"""GPU tests of the slice diagnostics: nbco_slice_moments / nbco_2d_slice_moments (Engine.slice_moments, slice_moments_2d) against
the fp64 numpy reference tests/slice_numpy.py -- at every size where the launch shape changes and every number of slices, on exact,
off-origin and degenerate data -- and the calls' contract: a slice's bytes do not depend on the other slices, a second call returns
the same bytes, the state is read only, refusals come before any launch, and a kd-tree evaluation's diagnostics stay as they were.

The bound on a sum field (mean, cov, m4) of a slice is that of test_gpu_beam_diag.py: 1e-10 x (mean absolute value of that sum's
terms within the slice), derived there for any summation order of at most 262 145 fp64 terms, which a slice never exceeds here.
n, min and max are exact; an empty slice is exact zeros; a one-particle slice has its particle as the mean and zeros elsewhere.

The reference costs one exactly rounded sum per field and slice in Python: 65 536 slices of the largest state take it eight to
twenty seconds, depending on the host; every other case takes at most three."""
import ctypes

import numpy as np
import pytest

import beam_numpy as BN
import slice_numpy as SN
import test_gpu_beam_diag as BD
from test_gpu_beam_diag import ball, head, dev, flat, check_moments

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 2, 4
DIMS = BD.DIMS
DTYPE = BD.DTYPE
X, Y, Z, VX, VY, VZ = range(6)
CHUNK = BD._const("slice_diag_kernels.hpp", "kSliceChunk")      # particles per workgroup of the two passes
BLOCK = BD._const("k_reduce.hip", "kBlock")
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 262145]
BINS = [1, 2, 3, 64, 1000, 65536]
COORDS = {3: [X, Y, Z, VX, VY, VZ], 2: [X, Y, VX, VY]}
SUMS = ("mean", "min", "max", "cov", "m4")


@pytest.fixture(scope="module")
def eng(engine_lib):
    import torch
    from coulomb_oscillators_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    e = Engine()
    yield e
    e.close()


def slice_fn(e, dim):
    return e.slice_moments if dim == 3 else e.slice_moments_2d


def check_slices(recs, outside, ref, ref_outside, dim, n, what):
    """every slice against the reference; returns the worst deviation of a sum in units of its mean absolute term"""
    assert outside == ref_outside, what
    assert len(recs) == len(ref) and sum(m.n for m in recs) + outside == n, what
    worst = 0.0
    for s, (m, r) in enumerate(zip(recs, ref)):
        if r["n"] <= 1:
            # an empty slice is zeros, a one-particle slice its particle and zeros: every field equals the reference
            assert m.n == r["n"] and m.dim == dim, (what, s)
            for k in SUMS + ("emit", "halo_q", "halo"):
                assert np.array_equal(np.array(getattr(m, k)), r[k]), (what, s, k)
        else:
            worst = max(worst, check_moments(m, r, dim, (what, s)))
    return worst


def test_the_chunk_is_a_whole_number_of_workgroup_passes():
    assert CHUNK % BLOCK == 0 and len(set(SIZES)) == len(SIZES) and BD.ONE_PASS + 1 == SIZES[-1]


# ---- launch shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", DIMS)
def test_slices_at_every_launch_shape(eng, dim, n, bins):
    """the correlated ball of the beam test, cut off-centre (mean - 1.3 sigma .. mean + 1.7 sigma of the whole ball), the slicing
    coordinates in turn along the sizes and along the numbers of slices: every slice and n_outside equal the reference"""
    coord = COORDS[dim][(SIZES.index(n) + BINS.index(bins)) % len(COORDS[dim])]
    axis = (coord, bins) + BD.ball_window(dim, coord)
    st = head(ball(dim), n)
    d = dev(st)
    recs, outside = slice_fn(eng, dim)(d, n, axis)
    ref, ref_outside = SN.slice_moments(st, dim, axis)
    worst = check_slices(recs, outside, ref, ref_outside, dim, n, (dim, n, axis))
    assert np.array_equal(d.cpu().numpy(), st.reshape(-1)), "the state was modified"
    print("dim %d n %d bins %d coord %d: worst deviation of a sum from the reference, in units of the mean absolute term: %.2e" % (dim, n, bins, coord, worst))


@pytest.mark.parametrize("dim", DIMS)
def test_one_slice_that_holds_everything(eng, dim):
    """bins = 1 and a window wider than the beam: the slice is several chunks; its record is within the bound of the reference and
    within twice the bound of beam_moments of the same state (each is within the bound of the exact sums)"""
    n = 3 * CHUNK + 5
    st = head(ball(dim), n)
    d = dev(st)
    recs, outside = slice_fn(eng, dim)(d, n, (X, 1, -100.0, 100.0))
    ref = BN.moments(st, dim)
    assert outside == 0 and len(recs) == 1
    print("worst deviation from the reference: %.2e" % check_moments(recs[0], ref, dim, "one slice"))
    whole = BD.moments_fn(eng, dim)(d, n)
    assert recs[0].n == whole.n and np.array_equal(np.array(recs[0].min), np.array(whole.min)) and np.array_equal(np.array(recs[0].max), np.array(whole.max))
    worst = 0.0
    for k in ("mean", "cov", "m4"):
        err, scale = np.abs(np.array(getattr(recs[0], k)) - np.array(getattr(whole, k))), ref["scale"][k]
        assert (err <= 2e-10 * scale).all(), (k, err.max())
        worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()))
    print("worst deviation from beam_moments: %.2e" % worst)


@pytest.mark.parametrize("dim", DIMS)
def test_slices_of_integer_pairs_are_exact(eng, dim):
    """x takes the integers -4 .. 3 (8 bins over [-4, 4)), and at every x the other coordinates come in +- pairs of small integers:
    every slice has a flat x, means of exactly 0 elsewhere and integer sums, so mean, cov and m4 equal the reference in every field.
    The slices hold 2 .. 2 CHUNK + 2 particles, interleaved in the state."""
    rng = np.random.default_rng([5, dim])
    pairs = [1, 5, BLOCK // 2, BLOCK // 2 + 1, 300, CHUNK // 2, CHUNK // 2 + 1, CHUNK + 1]
    rows = []
    for v, m in zip(range(-4, 4), pairs):
        h = rng.integers(-8, 9, size=(m, 2 * dim))
        h[:, 0] = 0
        both = np.concatenate([h, -h])
        both[:, 0] = v
        rows.append(both)
    q = rng.permutation(np.concatenate(rows))
    n = len(q)
    st = np.stack([q[:, :dim], q[:, dim:]]).astype(DTYPE[dim])
    axis = (X, 8, -4.0, 4.0)
    recs, outside = slice_fn(eng, dim)(dev(st), n, axis)
    ref, ref_outside = SN.slice_moments(st, dim, axis)
    assert outside == ref_outside == 0
    for s, (m, r) in enumerate(zip(recs, ref)):
        assert m.n == r["n"] == 2 * pairs[s]
        assert m.mean[0] == s - 4 and not np.array(m.mean)[1:].any()
        for k in SUMS:
            assert np.array_equal(np.array(getattr(m, k)), r[k]), (s, k)
        check_moments(m, r, dim, ("integer pairs", s))


@pytest.mark.parametrize("dim", DIMS)
def test_slices_of_a_beam_off_the_origin(eng, dim):
    """centre 1000, sigma of order 1 (fp32 in 3-D), 16 slices along the last position axis: the central form about the slice's own
    mean keeps the fourth moments within the bound"""
    n = 20000
    st = ball(dim, n, 2, 1000.0)
    coord = dim - 1
    axis = (coord, 16) + BD.window(st, dim, coord)
    recs, outside = slice_fn(eng, dim)(dev(st), n, axis)
    ref, ref_outside = SN.slice_moments(st, dim, axis)
    assert min(r["n"] for r in ref) > 100 and all(abs(r["mean"][0] - 1000.0) < 1.0 and 0.1 < r["m4"][0, 0] < 30.0 for r in ref)
    print("worst deviation: %.2e" % check_slices(recs, outside, ref, ref_outside, dim, n, "off-origin"))


# ---- independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_a_slice_does_not_depend_on_the_other_slices(eng, dim):
    """64 slices; then the particles of one slice alone, in their order, as one slice of a wide window: mean, min, max, cov and m4
    are the same bytes -- for the fullest slice (several chunks), one of a few particles and one in between.  And a NaN in y of one
    particle changes its slice's record and no other slice's bytes."""
    n = 100000
    st = np.array(head(ball(dim), n))
    coord = X
    q = st[0, :, coord].astype(np.float64)
    axis = (coord, 64, float(q.mean() - 1.3 * q.std()), float(q.mean() + 4.0 * q.std()))   # (the last slices lie in the tail)
    recs, _ = slice_fn(eng, dim)(dev(st), n, axis)
    rows, _ = SN.members(st, dim, axis)
    counts = np.array([len(r) for r in rows])
    assert counts.tolist() == [m.n for m in recs] and counts.max() > 2 * CHUNK
    order = np.argsort(counts, kind="stable")
    few = int(order[np.searchsorted(counts[order], 2)])
    picks = [int(order[-1]), few, int(order[len(order) // 2])]
    assert 2 <= counts[few] < BLOCK < counts[picks[2]] < counts[picks[0]]
    for s in picks:
        sub = np.ascontiguousarray(st[:, rows[s]])
        q = sub[0, :, coord].astype(np.float64)
        alone, outside = slice_fn(eng, dim)(dev(sub), len(rows[s]), (coord, 1, float(q.min()) - 1.0, float(q.max()) + 1.0))
        assert outside == 0 and alone[0].n == recs[s].n
        for k in SUMS:
            assert np.array(getattr(alone[0], k)).tobytes() == np.array(getattr(recs[s], k)).tobytes(), (s, k)
    victim = int(rows[picks[2]][7])
    st[0, victim, 1] = np.nan
    again, _ = slice_fn(eng, dim)(dev(st), n, axis)
    for s in range(64):
        same = flat(again[s]).tobytes() == flat(recs[s]).tobytes()
        assert same == (s != picks[2]), s
    assert np.isnan(again[picks[2]].mean[1]) and again[picks[2]].n == recs[picks[2]].n


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_slices_of_degenerate_shapes(eng, dim):
    """all particles coincident; the slicing axis itself flat; all velocities 0; a window that misses the beam; a NaN in the slicing
    coordinate: nothing is NaN, zeros are where the reference has them"""
    n = 1000
    base = np.array(ball(dim, n, 3))
    coincident = np.empty_like(base)
    coincident[0], coincident[1] = 0.3, -0.7
    flat_axis = base.copy()
    flat_axis[0, :, 0] = 0.3
    cold = base.copy()
    cold[1] = 0.0
    holed = base.copy()
    holed[0, 11, 0] = np.nan
    cases = (("coincident", coincident, (X, 4, 0.0, 1.0)), ("flat slicing axis", flat_axis, (X, 5, 0.0, 1.0)),
             ("cold", cold, (dim - 1, 7) + BD.window(cold, dim, dim - 1)), ("missed", base, (X, 9, 50.0, 60.0)),
             ("NaN on the slicing axis", holed, (X, 6, -100.0, 100.0)))
    for name, st, axis in cases:
        recs, outside = slice_fn(eng, dim)(dev(st), n, axis)
        ref, ref_outside = SN.slice_moments(st, dim, axis)
        assert all(np.isfinite(flat(m)).all() for m in recs), name
        check_slices(recs, outside, ref, ref_outside, dim, n, name)
        for m, r in zip(recs, ref):
            assert (np.array(m.cov)[r["cov"] == 0] == 0).all() and (np.array(m.m4)[r["m4"] == 0] == 0).all(), name
            for k in ("emit", "halo_q", "halo"):
                assert (np.array(getattr(m, k))[r[k] == 0] == 0).all(), (name, k)
        if name in ("coincident", "flat slicing axis"):
            assert [m.n for m in recs] == [0, n] + [0] * (axis[1] - 2) and outside == 0
            assert not np.array(recs[1].cov)[0].any() and recs[1].mean[0] == ref[1]["mean"][0] == np.float64(DTYPE[dim](0.3))
        if name == "coincident":
            assert not np.array(recs[1].cov).any() and not np.array(recs[1].m4).any() and np.array_equal(np.array(recs[1].mean), ref[1]["mean"])
        if name == "cold":
            assert all(not np.array(m.cov)[dim:].any() and not np.array(m.emit).any() for m in recs) and outside > 0
        if name == "missed":
            assert outside == n and all(m.n == 0 and m.dim == dim and not flat(m)[2:].any() for m in recs)
        if name == "NaN on the slicing axis":
            assert outside == 1 and sum(m.n for m in recs) == n - 1


# ---- contract --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_slices_contract(eng, dim):
    """a second call returns identical bytes; the state is unchanged byte for byte; a non-default stream and sync = 0 work; every
    refusal returns its status and leaves out_host and *n_outside_host as they were; a good call afterwards still works"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, HistAxis, Moments
    n = 5000
    st = head(ball(dim), n)
    d = dev(st)
    axis = (VX, 48) + BD.window(st, dim, VX)

    def call(e):
        recs, outside = slice_fn(e, dim)(d, n, axis)
        return bytes(recs), outside
    first = call(eng)
    assert call(eng) == first
    assert np.array_equal(d.cpu().numpy(), st.reshape(-1))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = Engine(sync=0)
        try:
            assert call(other) == first
        finally:
            other.close()

    fn = eng.lib.nbco_slice_moments if dim == 3 else eng.lib.nbco_2d_slice_moments
    out = (Moments * 8)()
    ctypes.memset(out, 0x5a, ctypes.sizeof(out))
    before = bytes(out)
    outside = ctypes.c_longlong(-7777)
    ptr = ctypes.c_void_p(d.data_ptr())

    def refused(buf, n_, ax, recs, cnt, status, why):
        arr = HistAxis(*ax) if ax is not None else None
        assert fn(eng.ctx, buf, n_, ctypes.byref(arr) if arr is not None else None, recs, ctypes.byref(cnt) if cnt is not None else None) == status, why
        assert bytes(out) == before and outside.value == -7777, why
    ok = (X, 8, -1.0, 1.0)
    nan, inf = float("nan"), float("inf")
    refused(None, n, ok, out, outside, ERR_ARG, "NULL buf")
    refused(ptr, n, None, out, outside, ERR_ARG, "NULL axis")
    refused(ptr, n, ok, None, outside, ERR_ARG, "NULL out")
    refused(ptr, n, ok, out, None, ERR_ARG, "NULL n_outside")
    refused(ptr, 0, ok, out, outside, ERR_ARG, "n = 0")
    refused(ptr, -1, ok, out, outside, ERR_ARG, "n < 0")
    refused(ptr, n, (-1, 8, -1.0, 1.0), out, outside, ERR_ARG, "coordinate -1")
    refused(ptr, n, (6, 8, -1.0, 1.0), out, outside, ERR_ARG, "coordinate 6")
    if dim == 2:
        refused(ptr, n, (Z, 8, -1.0, 1.0), out, outside, ERR_ARG, "Z in 2-D")
        refused(ptr, n, (VZ, 8, -1.0, 1.0), out, outside, ERR_ARG, "VZ in 2-D")
    refused(ptr, n, (X, 0, -1.0, 1.0), out, outside, ERR_ARG, "bins = 0")
    refused(ptr, n, (X, -4, -1.0, 1.0), out, outside, ERR_ARG, "bins < 0")
    refused(ptr, n, (X, 65537, -1.0, 1.0), out, outside, ERR_ARG, "bins > 65536")
    refused(ptr, n, (X, 8, nan, 1.0), out, outside, ERR_ARG, "lo NaN")
    refused(ptr, n, (X, 8, -1.0, nan), out, outside, ERR_ARG, "hi NaN")
    refused(ptr, n, (X, 8, -inf, 1.0), out, outside, ERR_ARG, "lo -inf")
    refused(ptr, n, (X, 8, -1.0, inf), out, outside, ERR_ARG, "hi inf")
    refused(ptr, n, (X, 8, 1.0, 1.0), out, outside, ERR_ARG, "lo = hi")
    refused(ptr, n, (X, 8, 1.0, -1.0), out, outside, ERR_ARG, "lo > hi")
    refused(ptr, 1 << 31, ok, out, outside, ERR_UNSUPPORTED, "n = 2^31")
    with pytest.raises(EngineError) as ei:
        slice_fn(eng, dim)(d, n, (X, 0, -1.0, 1.0))
    assert ei.value.status == ERR_ARG
    assert call(eng) == first


def test_slices_leave_a_kd_evaluation_as_it_was(oracle32):
    """a kd evaluation followed by slice_moments and slice_moments_2d, then energy_kd, energy_fmm and probe_kd: the bits they return
    without the slices in between; the slice records equal a fresh context's"""
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
        ax3, ax3big = (Z, 16, -0.015, 0.02), (VX, 4096, -0.005, 0.004)
        before = look()
        r3, o3 = e.slice_moments(d, n, ax3)
        r3big, o3big = e.slice_moments(d, n, ax3big)
        assert look() == before
        st2 = head(ball(2), 2500)
        d2 = dev(st2)
        ax2 = (Y, 5, -0.2, 0.3)
        r2, o2 = e.slice_moments_2d(d2, 2500, ax2)
        assert look() == before
        for got, want in (((r3, o3), fresh.slice_moments(d, n, ax3)), ((r3big, o3big), fresh.slice_moments(d, n, ax3big)),
                          ((r2, o2), fresh.slice_moments_2d(d2, 2500, ax2)), ((r3, o3), e.slice_moments(d, n, ax3))):
            assert bytes(got[0]) == bytes(want[0]) and got[1] == want[1]
        ref, ref_outside = SN.slice_moments(buf[:2], 3, ax3)
        check_slices(r3, o3, ref, ref_outside, 3, n, "initial state")
    finally:
        e.close()
        fresh.close()
