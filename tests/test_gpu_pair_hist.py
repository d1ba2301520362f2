"""GPU tests of the pair statistics: nbco_pair_hist / nbco_pair_hist_tree / nbco_2d_pair_hist (Engine.pair_hist, pair_hist_tree,
pair_hist_2d) against the fp64 numpy reference tests/pairstat_numpy.py.  The pair rule has no square root and no fused
multiply-add, counts are integers and a minimum is a minimum: every comparison is np.array_equal on the counts and on the BYTES of
nn2 -- there is no tolerance anywhere in this file.  The tree form must return the bytes of the exact form."""
import functools
import os
import re

import numpy as np
import pytest

import pairstat_numpy as PN
import shapes3d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coulomb_oscillators_amd", "csrc")
ERR_ARG, ERR_UNSUPPORTED = 2, 4
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
BINS = (1, 2, 64, 1000)
RMAX = (0.0005, 0.002, 1.0)     # on the reference ball: 0.04 %, 2 % and 100 % of the pairs inside; median nearest neighbour 4.5e-4
GARBAGE_COUNT, GARBAGE_NN2 = -7777, -123.456
LDS_BINS = int(re.search(r"constexpr int kHistLdsBins = (\d+);", open(os.path.join(CSRC, "beam_diag_kernels.hpp")).read()).group(1))


@pytest.fixture(scope="module")
def eng(engine_lib):
    import torch
    from coulomb_oscillators_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    e = Engine()
    yield e
    e.close()


_BALL = {}


def ball(oracle32, dim):
    """positions of the reference ball at n = 4097: float32 xyz, or for 2-D its xy columns as float64 with the low mantissa bits
    filled (so that the fp64 loads matter)"""
    if not _BALL:
        b3 = np.ascontiguousarray(oracle32.init_reference(SIZES[-1])[0])
        b2 = b3[:, :2].astype(np.float64) * (1.0 + 1e-9 * np.random.default_rng(2).standard_normal((len(b3), 2)))
        for b in (b3, b2):
            b.setflags(write=False)
        _BALL[3], _BALL[2] = b3, b2
    return _BALL[dim]


@functools.lru_cache(maxsize=None)
def _ball_inside(dim, n, rmax):
    return PN.inside_pairs(_BALL[dim][:n], rmax)


def ball_reference(oracle32, dim, n, bins, rmax):
    ball(oracle32, dim)
    r2, nn2 = _ball_inside(dim, n, rmax)
    return PN.counts_of(r2, n, bins, rmax), nn2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def fn_of(e, form):
    return dict(exact=e.pair_hist, tree=e.pair_hist_tree, exact2d=e.pair_hist_2d)[form]


def run(e, form, d, n, bins, rmax, want_counts=True, want_nn2=True):
    """one call into buffers pre-filled with garbage; returns (counts or None, nn2 or None) as numpy arrays"""
    import torch
    counts = torch.full((bins + 1,), GARBAGE_COUNT, dtype=torch.int64, device="cuda") if want_counts else False
    nn2 = torch.full((n,), GARBAGE_NN2, dtype=torch.float64, device="cuda") if want_nn2 else None
    fn_of(e, form)(d, n, bins, rmax, counts=counts, nn2=nn2)
    return (counts.cpu().numpy() if want_counts else None), (nn2.cpu().numpy() if want_nn2 else None)


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "counts", got[0][:8], want[0][:8])
    assert got[1].tobytes() == want[1].tobytes(), (what, "nn2", np.flatnonzero(got[1] != want[1])[:8])


# ---- launch shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", SIZES)
def test_exact_forms_at_every_launch_shape(eng, oracle32, dim, n):
    """heads of one ball: below, at and above a wave, a tile and a workgroup, several tiles with a ragged last one; empty, sparse and
    full windows; one bin to a thousand.  The input is not written."""
    pos = ball(oracle32, dim)[:n]
    d = dev(pos)
    form = "exact" if dim == 3 else "exact2d"
    for rmax in RMAX:
        for bins in BINS:
            want = ball_reference(oracle32, dim, n, bins, rmax)
            got = run(eng, form, d, n, bins, rmax)
            same(got, want, (rmax, bins))
            assert got[0].sum() == n * (n - 1) // 2
    assert np.array_equal(d.cpu().numpy(), pos)
    if n == SIZES[-1] and dim == 3:
        nn = ball_reference(oracle32, 3, n, 1, RMAX[0])[1]
        assert np.isinf(nn).any() and np.isfinite(nn).any()   # the smallest window is a mix, as the module's table says


@pytest.mark.parametrize("bins", [LDS_BINS, LDS_BINS + 1, 65536])
def test_histogram_storage(eng, oracle32, bins):
    """the last count of bins in LDS, the first straight to the global counts, and the most the call takes; tree and exact forms"""
    n = 1000
    d3, d2 = dev(ball(oracle32, 3)[:n]), dev(ball(oracle32, 2)[:n])
    for rmax in RMAX[1:]:
        want = ball_reference(oracle32, 3, n, bins, rmax)
        same(run(eng, "exact", d3, n, bins, rmax), want, rmax)
        same(run(eng, "tree", d3, n, bins, rmax), want, rmax)
        same(run(eng, "exact2d", d2, n, bins, rmax), ball_reference(oracle32, 2, n, bins, rmax), rmax)


# ---- tree = exact = reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65, 3000, 4097])
def test_tree_is_exact_is_reference_on_the_ball(eng, oracle32, n):
    d = dev(ball(oracle32, 3)[:n])
    for rmax in RMAX:
        for bins in (1, 64):
            want = ball_reference(oracle32, 3, n, bins, rmax)
            same(run(eng, "exact", d, n, bins, rmax), want, ("exact", rmax, bins))
            same(run(eng, "tree", d, n, bins, rmax), want, ("tree", rmax, bins))


def _shape_n(name):
    return 3375 if name == "lattice" else 4096 if name.startswith("dup") else 4001


@pytest.mark.parametrize("shape", shapes3d.SHAPES)
def test_tree_is_exact_is_reference_on_every_shape(eng, oracle32, shape):
    """flat, collinear, tied, duplicated, stretched and late-run inputs: tied coordinates settle the tree build by demotion, duplicated
    points are pairs at r2 = 0.  The three windows are those of the ball, scaled by the shape's extent (the longest side of its
    bounding box) over the ball's."""
    n = _shape_n(shape)
    pos = np.ascontiguousarray(shapes3d.state(oracle32, shape, n)[0])
    gauss = shapes3d.state(oracle32, "gauss", n)[0]
    scale = float((pos.max(0) - pos.min(0)).max() / (gauss.max(0) - gauss.min(0)).max())
    d = dev(pos)
    for rmax in RMAX:
        want = PN.pair_hist(pos, 64, rmax * scale)
        same(run(eng, "exact", d, n, 64, rmax * scale), want, ("exact", rmax))
        same(run(eng, "tree", d, n, 64, rmax * scale), want, ("tree", rmax))


def test_tree_is_exact_at_20000_whatever_the_tree(engine_lib, oracle32):
    """no numpy: the two forms against each other at bins = 256, then the tree form with a deep tree, a shallow tree and another
    dens_inhom -- the tree decides only what is skipped, so nothing may move"""
    from coulomb_oscillators_amd import Engine
    n, bins = 20000, 256
    d = dev(np.ascontiguousarray(oracle32.init_reference(n)[0]))
    e = Engine()
    try:
        for rmax in RMAX[:2]:
            want = run(e, "exact", d, n, bins, rmax)
            assert want[0].sum() == n * (n - 1) // 2 and 0 < want[0][:bins].sum()
            same(run(e, "tree", d, n, bins, rmax), want, "default tree")
            # (tree_L = 3: 2500 per leaf, the shallowest tree the build holds at this n -- its LDS slice takes 4096 per leaf)
            for opts in (dict(tree_L=12), dict(tree_L=3), dict(tree_L=0, dens_inhom=8.0), dict(tree_L=0, dens_inhom=0.25, fmm_order=6)):
                e.set(**opts)
                same(run(e, "tree", d, n, bins, rmax), want, opts)
            e.set(tree_L=0, dens_inhom=1.0, fmm_order=3)
    finally:
        e.close()


# ---- degenerate ------------------------------------------------------------------------------------------------------------------------
def test_coincident_particles(eng):
    """20000 particles in one point, both forms: every lane of every wave adds to one bin; nn2 = 0"""
    n = 20000
    d = dev(np.full((n, 3), 0.00123, dtype=np.float32))
    for form in ("exact", "tree"):
        for bins in (1, 64):
            c, m = run(eng, form, d, n, bins, 1e-3)
            assert c[0] == n * (n - 1) // 2 and not c[1:].any(), (form, bins)
            assert (m == 0.0).all()
    d2 = dev(np.full((n, 2), -0.5))
    c, m = run(eng, "exact2d", d2, n, 64, 1e-3)
    assert c[0] == n * (n - 1) // 2 and not c[1:].any() and (m == 0.0).all()


def test_one_bin_beyond_32_bits(eng):
    """93000 coincident particles, exact form: one bin holds 4.32e9 > 2^32 pairs -- a 32-bit counter anywhere would wrap"""
    n = 93000
    d = dev(np.zeros((n, 3), dtype=np.float32))
    c, _ = run(eng, "exact", d, n, 64, 1e-3, want_nn2=False)
    assert n * (n - 1) // 2 > 1 << 32
    assert c[0] == n * (n - 1) // 2 and not c[1:].any()


def test_integer_lattice(eng):
    """exact distances on bin edges: r = 0.5 k belongs to bin k, r = rmax is outside (tests/test_pairstat_host.py has the host side)"""
    pos, want = PN.lattice()
    n = len(pos)
    d = dev(pos)
    for form in ("exact", "tree"):
        c, m = run(eng, form, d, n, PN.LATTICE_BINS, PN.LATTICE_RMAX)
        assert np.array_equal(c, want), form
        assert (m == 1.0).all()


def test_a_nan_coordinate_is_outside(eng, oracle32):
    n = 1000
    pos = ball(oracle32, 3)[:n].copy()
    want = ball_reference(oracle32, 3, n, 64, RMAX[1])
    pos[417, 1] = np.nan
    c, m = run(eng, "exact", dev(pos), n, 64, RMAX[1])
    ref = PN.pair_hist(pos, 64, RMAX[1])
    same((c, m), ref)
    keep = np.arange(n) != 417
    assert np.isinf(m[417]) and c[64] >= n - 1
    rest = PN.pair_hist(pos[keep], 64, RMAX[1])
    assert np.array_equal(c[:64], rest[0][:64]) and m[keep].tobytes() == rest[1].tobytes()
    assert c[:64].sum() < want[0][:64].sum()


# ---- contract -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["exact", "tree", "exact2d"])
def test_repeatable_and_single_outputs(eng, oracle32, form):
    """a second call returns the same bytes; counts only and nn2 only return what both together return; counts=None allocates"""
    n, bins, rmax = 3000, 64, RMAX[1]
    dim = 2 if form == "exact2d" else 3
    d = dev(ball(oracle32, dim)[:n])
    want = ball_reference(oracle32, dim, n, bins, rmax)
    first, second = run(eng, form, d, n, bins, rmax), run(eng, form, d, n, bins, rmax)
    same(first, want)
    same(second, first)
    c, none = run(eng, form, d, n, bins, rmax, want_nn2=False)
    assert none is None and np.array_equal(c, want[0])
    none, m = run(eng, form, d, n, bins, rmax, want_counts=False)
    assert none is None and m.tobytes() == want[1].tobytes()
    none, m = run(eng, form, d, n, -5, rmax, want_counts=False)      # bins is ignored without counts
    assert m.tobytes() == want[1].tobytes()
    made = fn_of(eng, form)(d, n, bins, rmax)
    assert made.dtype.is_floating_point is False and made.numel() == bins + 1 and np.array_equal(made.cpu().numpy(), want[0])


@pytest.mark.parametrize("form", ["exact", "tree", "exact2d"])
def test_non_default_stream_without_sync(engine_lib, oracle32, form):
    import torch
    from coulomb_oscillators_amd import Engine
    n, bins, rmax = 3000, 64, RMAX[1]
    dim = 2 if form == "exact2d" else 3
    want = ball_reference(oracle32, dim, n, bins, rmax)
    d = dev(ball(oracle32, dim)[:n])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    e = Engine(stream=s.cuda_stream, sync=0)
    try:
        with torch.cuda.stream(s):
            counts = torch.full((bins + 1,), GARBAGE_COUNT, dtype=torch.int64, device="cuda")
            nn2 = torch.full((n,), GARBAGE_NN2, dtype=torch.float64, device="cuda")
            fn_of(e, form)(d, n, bins, rmax, counts=counts, nn2=nn2)
        s.synchronize()
        same((counts.cpu().numpy(), nn2.cpu().numpy()), want)
    finally:
        e.close()


@pytest.mark.parametrize("form", ["exact", "tree", "exact2d"])
def test_refusals_leave_the_outputs_alone(eng, oracle32, form):
    import torch
    from coulomb_oscillators_amd import EngineError
    from coulomb_oscillators_amd.engine import _ptr
    n, bins, rmax = 1000, 64, RMAX[1]
    dim = 2 if form == "exact2d" else 3
    d = dev(ball(oracle32, dim)[:n])
    counts = torch.full((bins + 1,), GARBAGE_COUNT, dtype=torch.int64, device="cuda")
    nn2 = torch.full((n,), GARBAGE_NN2, dtype=torch.float64, device="cuda")
    fn = getattr(eng.lib, dict(exact="nbco_pair_hist", tree="nbco_pair_hist_tree", exact2d="nbco_2d_pair_hist")[form])

    def call(ctx=eng.ctx, p=d, n=n, bins=bins, rmax=rmax, c=counts, m=nn2):
        return fn(ctx, _ptr(p), n, bins, rmax, _ptr(c), _ptr(m))
    tiny = 1e-160                                   # width^2 = (1e-160 / 64)^2 underflows below DBL_MIN
    bad = [dict(ctx=None), dict(p=None), dict(n=0), dict(n=-3), dict(c=None, m=None), dict(rmax=0.0), dict(rmax=-1.0),
           dict(rmax=float("inf")), dict(rmax=float("nan")), dict(bins=0), dict(bins=-1), dict(bins=65537), dict(rmax=tiny)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert call(n=1 << 31) == ERR_UNSUPPORTED
    if form == "tree":
        assert call(n=(0x7fffffff // 4) + 1) == ERR_UNSUPPORTED
    assert call(rmax=tiny, c=None) in (0,)           # without counts the bins and their width are not looked at
    assert (nn2 == float("inf")).all()               # (nothing is within 1e-160)
    nn2.fill_(GARBAGE_NN2)
    for kw in bad[1:]:
        call(**kw)
    torch.cuda.synchronize()
    assert (counts == GARBAGE_COUNT).all() and (nn2 == GARBAGE_NN2).all()
    with pytest.raises(EngineError) as err:
        fn_of(eng, form)(d, n, 0, rmax)
    assert err.value.status == ERR_ARG
    # a good call afterwards
    same(run(eng, form, d, n, bins, rmax), ball_reference(oracle32, dim, n, bins, rmax))


def test_tree_form_refuses_leaves_the_build_cannot_hold(engine_lib, oracle32):
    """tree_L = 2 at n = 20000 asks for 5000 particles per leaf, more than the build's LDS slice: NBCO_ERR_UNSUPPORTED before any
    launch, the outputs untouched, and the exact form does not care"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError
    n, bins, rmax = 20000, 64, RMAX[0]
    d = dev(np.ascontiguousarray(oracle32.init_reference(n)[0]))
    e = Engine(tree_L=2)
    try:
        counts = torch.full((bins + 1,), GARBAGE_COUNT, dtype=torch.int64, device="cuda")
        nn2 = torch.full((n,), GARBAGE_NN2, dtype=torch.float64, device="cuda")
        with pytest.raises(EngineError) as err:
            e.pair_hist_tree(d, n, bins, rmax, counts=counts, nn2=nn2)
        assert err.value.status == ERR_UNSUPPORTED and "per leaf" in str(err.value)
        assert (counts == GARBAGE_COUNT).all() and (nn2 == GARBAGE_NN2).all()
        want = run(e, "exact", d, n, bins, rmax)
        e.set(tree_L=0)
        same(run(e, "tree", d, n, bins, rmax), want)
    finally:
        e.close()


# ---- state -------------------------------------------------------------------------------------------------------------------------------
def test_pair_statistics_leave_a_kd_evaluation_as_it_was(oracle32):
    """a kd evaluation, then energy_kd, energy_fmm and probe_kd: the same bytes before and after all three new calls; nbco_kd_get_info
    unchanged; and the new calls return what a fresh context returns"""
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
            return got.tobytes() + bytes(e.kd_info())
        d2 = dev(ball(oracle32, 2)[:2500])
        before = look()
        got3 = run(e, "exact", d, n, 64, RMAX[1])
        assert look() == before
        gott = run(e, "tree", d, n, 64, RMAX[1])
        assert look() == before
        got2 = run(e, "exact2d", d2, 2500, 64, RMAX[1])
        assert look() == before
        want = PN.pair_hist(buf[0], 64, RMAX[1])
        same(got3, want)
        same(gott, want)
        same(run(fresh, "tree", d, n, 64, RMAX[1]), want)
        same(got2, run(fresh, "exact2d", d2, 2500, 64, RMAX[1]))
    finally:
        e.close()
        fresh.close()


def test_tree_form_between_tree_diagnostics(oracle32):
    """energy_tree -> pair_hist_tree -> energy_tree -> probe_tree on one context (they share the private context): each returns what
    it returns without the call in the middle"""
    import torch
    from coulomb_oscillators_amd import Engine
    n = 4096
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    d, prm = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda()
    t = torch.from_numpy(np.ascontiguousarray(buf[0][:200] * np.float32(1.2))).cuda()

    def drive(with_pairs):
        e = Engine(fmm_order=4)
        try:
            out = []
            phi = torch.zeros(n, dtype=torch.float64, device="cuda")
            out.append(np.asarray(e.energy_tree(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes())
            pairs = run(e, "tree", d, n, 64, RMAX[1]) if with_pairs else None
            out.append(np.asarray(e.energy_tree(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes())
            a = torch.zeros((200, 3), dtype=torch.float64, device="cuda")
            psi = torch.zeros(200, dtype=torch.float64, device="cuda")
            e.probe_tree(d, n, t, 200, prm, a, psi)
            out.append(a.cpu().numpy().tobytes() + psi.cpu().numpy().tobytes())
            return out, pairs
        finally:
            e.close()
    plain, _ = drive(False)
    mixed, pairs = drive(True)
    assert plain == mixed
    same(pairs, PN.pair_hist(buf[0], 64, RMAX[1]))
