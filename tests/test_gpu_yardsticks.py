"""The kernels the rest of the suite is measured with -- nbco_direct / nbco_direct3, nbco_energy, the step / elastic / gather
kernels, nbco_integrate, the reductions -- against fp64 at every launch shape they have: more than one source tile per j-split of
the direct sum (the prefetch path), softened and coincident and badly conditioned inputs, the tile edges of the energy reduction,
second and third grid-stride passes of the reductions and the stream kernels, misaligned and mixed-alignment arguments, and the
integrators at a step where their constants show.

Every expected value comes from oracle64 or from numpy in fp64 on the same fp32 inputs.  Where a bound is "k x the reference's
own error", that error (oracle32 against the same fp64 result) is measured inside the test and printed beside the kernel's (run
with -s); the reference floors quoted in the comments are from the gcc build of the oracle on x86-64."""
import numpy as np
import pytest

import integrators3d_numpy as ig
from direct_numpy import K_TILE, direct3_rows_fp32, direct_launch_shape, direct_rows_fp64, find_n, same_bits
from nbutil import force_err

pytestmark = pytest.mark.gpu

THREADS = 8


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def f32(v):
    """the value a float option or argument has once it crossed the C ABI"""
    return float(np.float32(v))


# ---- A. direct sums at every launch shape -------------------------------------------------------------------------------------
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def gpu_direct(engine, pos, par, kahan):
    import torch
    p = dev(pos)
    a = torch.empty_like(p)
    (engine.direct3 if kahan else engine.direct)(p, a, len(pos), dev(par))
    return a.cpu().numpy()


def direct_figures(engine, oracle32, oracle64, pos, par, eps2=1e-18, rows=None, label=""):
    """errors against fp64 of: GPU direct, GPU direct3, the reference's Kahan sum (oracle32.direct3); and the GPU results"""
    n = len(pos)
    eps2 = f32(eps2)
    if rows is None:
        rows = slice(None)
        want = oracle64.direct3(pos.astype(np.float64), par.astype(np.float64), eps2=eps2, threads=THREADS)
        ref32 = oracle32.direct3(pos, par, eps2=eps2, threads=THREADS)
    else:
        want = direct_rows_fp64(pos, rows, float(par[0]), eps2)
        ref32 = direct3_rows_fp32(pos, rows, par[0], eps2)
    a, a3 = gpu_direct(engine, pos, par, False), gpu_direct(engine, pos, par, True)
    assert np.isfinite(a).all() and np.isfinite(a3).all()
    fig = dict(direct=force_err(a[rows], want), direct3=force_err(a3[rows], want), floor3=force_err(ref32, want))
    print("%s n=%d eps2=%.0e: direct %.2e  direct3 %.2e  oracle32.direct3 %.2e  (all against fp64)"
          % (label, n, eps2, fig["direct"], fig["direct3"], fig["floor3"]))
    return fig, a, a3, want


def assert_direct3_rule(fig):
    """GPU direct3 at most 4 x the reference's Kahan sum (v_rsq_f32 and the 16-source fold), never above 1e-6"""
    assert fig["direct3"] <= min(4 * fig["floor3"], 1e-6), fig


SHAPES = [
    # name, the n of 256 CUs, the shape it is there for
    ("last_split_one_partial_tile", 20003, lambda s, tps, last, src: tps >= 2 and last == 1 and 1 <= src & 3 and src >= 4 and src < K_TILE),
    ("partial_tile_through_prefetch", 20259, lambda s, tps, last, src: tps >= 2 and last >= 2 and 1 <= src & 3 and src >= 4 and src < K_TILE),
]


@pytest.mark.parametrize("name,n256,want", SHAPES, ids=[s[0] for s in SHAPES])
def test_direct_with_prefetch_against_fp64(engine, oracle32, oracle64, name, n256, want):
    """tiles_per_split >= 2: the double-buffered prefetch runs; a short last split; a partial last tile (quads + scalar tail) that is
    a split's only tile, or arrives through the prefetch.
    Reference floor: oracle32.direct3 against fp64 1.8e-07 at n = 20003 (the kernel's own comment claims 2e-07), so direct3 is held
    to 7.4e-07 there."""
    cus = num_cu()
    n = n256 if cus == 256 else find_n(cus, want, 16385, 40000)
    shape = direct_launch_shape(n, cus)
    assert want(*shape), "n = %d no longer reaches '%s' on %d CUs: %s" % (n, name, cus, shape)
    if cus == 256:
        assert shape == {20003: (40, 2, 1, 35), 20259: (40, 2, 2, 35)}[n]
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    fig, _, _, _ = direct_figures(engine, oracle32, oracle64, pos, par, label=name)
    assert fig["direct"] < 1e-5
    assert_direct3_rule(fig)


def test_direct_many_tiles_per_split_against_fp64_rows(engine, oracle32):
    """tiles_per_split 17 on 256 CUs (n = 65573): the tile buffers alternate many times, the last split has two tiles and the last
    tile 37 sources.  256 rows against the fp64 direct sum, among them the first and the last particle and both sides of the first
    target-block edge.  Reference floor: the reference's Kahan sum restated for these rows (direct_numpy.direct3_rows_fp32, bit for
    bit oracle32.direct3) is 5.6e-08 from fp64 on them, so direct3 is held to 2.2e-07."""
    cus = num_cu()
    want = lambda s, tps, last, src: tps >= 8 and 2 <= last < tps and 1 <= src & 3 and src >= 4 and src < K_TILE
    n = 65573 if cus == 256 else find_n(cus, want, 50000, 90000)
    shape = direct_launch_shape(n, cus)
    assert want(*shape), "n = %d no longer reaches many tiles per split on %d CUs: %s" % (n, cus, shape)
    if cus == 256:
        assert shape == (16, 17, 2, 37)
    must = np.array([0, 1023, 1024, n - 1])
    rest = np.random.default_rng(5).permutation(n)
    rows = np.concatenate([must, rest[~np.isin(rest, must)][:252]])
    assert len(np.unique(rows)) == 256
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    fig, _, _, _ = direct_figures(engine, oracle32, None, pos, par, rows=rows, label="many_tiles_per_split")
    assert fig["direct"] < 1e-5
    assert_direct3_rule(fig)


@pytest.mark.parametrize("n", [3, 5, 6, 7, 257, 258, 259])
def test_direct_scalar_tails_against_fp64(engine, oracle32, oracle64, n):
    """jcount & 3 in {1, 2, 3}, in a first tile (with 0 or 1 quads before it) and in a second tile that is nothing but the tail.
    Reference floors: oracle32.direct3 against fp64 6.0e-08, 7.0e-08, 7.2e-08, 8.5e-08, 1.3e-07, 1.3e-07, 9.8e-08 in the order of n."""
    splits, tps, last, src = direct_launch_shape(n, num_cu())
    assert (splits, tps, last) == ((n + K_TILE - 1) // K_TILE, 1, 1) and src & 3 == n & 3 != 0 and src == (n if n < K_TILE else n - K_TILE)
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    fig, _, _, _ = direct_figures(engine, oracle32, oracle64, pos, par, label="scalar_tail")
    assert fig["direct"] < 1e-5
    assert_direct3_rule(fig)


def test_direct_with_prefetch_is_bit_reproducible(engine, oracle32):
    cus = num_cu()
    n = 20003 if cus == 256 else find_n(cus, SHAPES[0][2], 16385, 40000)
    assert direct_launch_shape(n, cus)[1] >= 2
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    for kahan in (False, True):
        first = gpu_direct(engine, pos, par, kahan)
        gpu_direct(engine, pos[::-1].copy(), par, not kahan)            # other contents in the partial-sum buffer in between
        assert same_bits(first, gpu_direct(engine, pos, par, kahan)), "direct3" if kahan else "direct"


# ---- B. softening, coincident and badly conditioned inputs ----------------------------------------------------------------------
def clumps():
    """8192 particles in 8 clumps of width 1e-5 whose centres are 3e-3 apart: neighbours 300 times closer than the cloud is wide"""
    rng = np.random.default_rng(1)
    n = 8192
    centres = rng.normal(0, 3e-3, (8, 3))
    x = (centres[rng.integers(0, 8, n)] + rng.normal(0, 1e-5, (n, 3))).astype(np.float32)
    v = rng.normal(0, 1e-3, (n, 3)).astype(np.float32)
    return x, v


def cloud(kind):
    x, v = clumps()
    if kind == "offset_clumps":
        x = x + np.float32(1.0)
    elif kind == "duplicates":
        x[1] = x[0]
        x[100:164] = x[99]
    return x, v


CLOUDS = [("clumps", 1e-18), ("offset_clumps", 1e-18), ("duplicates", 1e-18), ("duplicates", 1e-10), ("duplicates", 1e-6)]


@pytest.mark.parametrize("kind,eps2", CLOUDS, ids=["%s-%g" % c for c in CLOUDS])
def test_direct_on_clustered_and_coincident_clouds(engine, oracle32, oracle64, kind, eps2):
    """direct3 within 4 x the reference's Kahan sum; plain direct within the larger of 1e-5 and what the reference's plain fp32 sum
    (oracle32.direct2) keeps on the same input; coincident particles: finite, bit-identical accelerations; the energy reduction
    against fp64 on the same cloud.
    Reference floors against fp64 (oracle32.direct3 / oracle32.direct2):
        clumps         eps2 1e-18   1.5e-07 / 5.5e-05          duplicates  eps2 1e-18   1.6e-07 / 5.5e-05
        offset clumps  eps2 1e-18   1.5e-07 / 6.5e-05          duplicates  eps2 1e-10   6.6e-08 / 2.6e-05
                                                               duplicates  eps2 1e-06   6.1e-08 / 2.5e-06
    The plain fp32 sum of the reference does not keep 1e-5 on clumps: hence the larger of the two for plain direct."""
    x, v = cloud(kind)
    n = len(x)
    par = oracle32.params(n)
    engine.set(eps2=eps2)
    fig, a, a3, want = direct_figures(engine, oracle32, oracle64, x, par, eps2=eps2, label=kind)
    floor2 = force_err(oracle32.direct2(x, par, eps2=f32(eps2), threads=THREADS), want)
    print("%s eps2=%.0e: oracle32.direct2 against fp64 %.2e" % (kind, eps2, floor2))
    assert_direct3_rule(fig)
    assert fig["direct"] <= max(1e-5, floor2), (fig, floor2)
    if kind == "duplicates":
        for got in (a, a3):
            assert same_bits(got[1], got[0])
            assert same_bits(got[100:164], np.broadcast_to(got[99], (64, 3)))
    # the energy of the same cloud (test_energy_matches_fp64_direct_sum's tolerances)
    buf = np.stack([x, v, np.zeros_like(x)])
    e_want = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), eps2=f32(eps2), threads=THREADS)
    e_got = engine.energy(dev(buf), n, dev(par))
    print("%s eps2=%.0e: energy %r against %r, coulomb off by %.2e" % (kind, eps2, e_got, list(e_want), abs(e_got[2] - e_want[2]) / e_want[2]))
    np.testing.assert_allclose(e_got[:2], e_want[:2], rtol=1e-12)
    np.testing.assert_allclose(e_got[2], e_want[2], rtol=2e-6)


# ---- C. nbco_energy at the tile edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_energy_at_the_tile_edges(engine, oracle32, oracle64, n):
    """one particle (no pair at all), one pair, a tile short by one, a full tile, last tiles of one particle (257, 513: there the
    only term of the last tile is the excluded t + k == i one for the particle itself)"""
    buf = np.ascontiguousarray(oracle32.init_reference(max(n, 2))[:, :n])
    par = oracle32.params(n)
    want = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), eps2=f32(1e-18), threads=2)
    d, prm = dev(buf), dev(par)
    got = engine.energy(d, n, prm)
    np.testing.assert_allclose(got[:2], want[:2], rtol=1e-12)
    np.testing.assert_allclose(got[2], want[2], rtol=2e-6)
    if n == 1:
        assert got[2] == 0.0 and want[2] == 0.0
    else:
        assert got[2] > 0
    assert engine.energy(d, n, prm) == got                                  # the same bits


# ---- D. reductions beyond one grid pass -------------------------------------------------------------------------------------------
N_RED = 2 * 262144 + 77            # 1024 blocks x 256 threads cover 262144: the first 77 threads make three passes
PLANTS = [0, 63, 64, 255, 256, 262143, 262144, 524288, N_RED - 1]     # wave, block and grid-pass edges, both ends


def test_minmax_over_three_grid_passes(engine):
    x = np.random.default_rng(11).uniform(-0.999, 0.999, (N_RED, 3)).astype(np.float32)
    d = dev(x)

    def check(plants):
        h = x.copy()
        for i, c, val in plants:
            h[i, c] = val
            d[i, c] = val
        got = engine.minmax(d, N_RED).cpu().numpy()
        for i, c, _ in plants:
            d[i, c] = float(x[i, c])
        np.testing.assert_array_equal(got, np.stack([h.min(0), h.max(0)]), err_msg=repr(plants))

    check([])
    for k, i in enumerate(PLANTS):
        check([(i, k % 3, 7.0)])
        check([(i, (k + 1) % 3, -7.0)])
    # a different plant behind each of the six outputs
    check([(63, 0, -7.0), (262144, 1, -8.0), (N_RED - 1, 2, -9.0), (524288, 0, 7.0), (0, 1, 8.0), (262143, 2, 9.0)])


def test_pow_sum_counts_every_element_once(engine):
    """all ones: the sum is the number of elements; all zeros but one 3.0: the sum is 3^expo in its component -- exact in fp64, so an
    element counted twice or dropped shows.  (expo = 0 counts elements whatever they hold, x^0 = 1, so there the single 3.0 changes
    nothing and the sum is n.)"""
    import torch
    ones = torch.ones((N_RED, 3), dtype=torch.float32, device="cuda")
    for expo in (0, 1, 2, 3):
        assert engine.pow_sum(ones, expo, N_RED) == [float(N_RED)] * 3, expo
    z = torch.zeros((N_RED, 3), dtype=torch.float32, device="cuda")
    for k, i in enumerate(PLANTS):
        c = k % 3
        z[i, c] = 3.0
        for expo in (0, 1, 2, 3):
            want = [float(N_RED)] * 3 if expo == 0 else [3.0 ** expo if cc == c else 0.0 for cc in range(3)]
            assert engine.pow_sum(z, expo, N_RED) == want, (i, expo)
        z[i, c] = 0.0


def test_mean_relerr_over_three_grid_passes(engine):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((N_RED, 3)).astype(np.float32)
    ref = (x + 1e-3 * rng.standard_normal((N_RED, 3))).astype(np.float32)

    def formula(x, ref):            # reductions.cuh:37-42 in fp64
        x, ref = x.astype(np.float64), ref.astype(np.float64)
        return float(np.sqrt(np.maximum(((x - ref) ** 2).sum(1) / ((ref ** 2).sum(1) + 1e-18), 0)).mean())

    dx, dref = dev(x), dev(ref)
    want = formula(x, ref)
    got = engine.mean_relerr(dx, dref, N_RED)
    print("mean_relerr %.9e against %.9e" % (got, want))
    assert abs(got - want) <= 2e-5 * want + 1e-12
    assert engine.mean_relerr(dx, dx, N_RED) == 0.0
    for i in (0, 262144, N_RED - 1):            # a reference row of zeros: the 1e-18 keeps the quotient finite
        ref0 = ref.copy()
        ref0[i] = 0
        got = engine.mean_relerr(dx, dev(ref0), N_RED)
        assert np.isfinite(got) and got > want


# ---- E. stream kernels beyond one grid pass and off alignment -----------------------------------------------------------------------
N_STREAM = 2100003                 # 2048 blocks x 256 threads cover 524288 items; n mod 4 = 3 and 3n mod 4 = 1: both scalar tails
DS = f32(0.37)
K3 = np.array([1.2, 0.9, 1.1], dtype=np.float32)


def assert_correctly_rounded(got, exact, what):
    """|got - exact| <= half a unit in the last place of got (exact: fp64 from the fp32 inputs, itself good to 2^-53)"""
    got64 = got.astype(np.float64)
    slack = 0.5 * np.spacing(np.abs(got)).astype(np.float64) * (1 + 2.0 ** -20)
    bad = np.flatnonzero(~(np.abs(got64 - exact) <= slack))
    assert bad.size == 0, "%s: %d elements not correctly rounded, first at %d: got %r exact %r" % (what, bad.size, bad[0], got.ravel()[bad[0]], exact.ravel()[bad[0]])


def expected(op, b, a, k):
    """(exact or None, fp32 value or None) of the flat arrays after op; b: the array read, a: the array written"""
    b64, a64 = b.astype(np.float64), a.astype(np.float64)
    k3 = np.ones(3, np.float32) if k is None else k
    kk = np.tile(k3, len(b) // 3)
    if op == "step":
        return a64 + np.float64(np.float32(DS)) * b64, None          # a += b ds
    if op == "add_elastic":
        return a64 - kk.astype(np.float64) * b64, None                # a -= k o p
    if op == "elastic":
        return None, -(kk * b)                                        # a = -k o p
    if op == "rescale":
        return None, a * np.float32(0.37)
    raise ValueError(op)


def run_stream(engine, op, n, shift_read=0, shift_write=0, seed=0, k=K3):
    """run one kernel on arrays that sit `shift` floats into an aligned buffer with guard floats around them"""
    import torch
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(3 * n).astype(np.float32)        # read
    a = rng.standard_normal(3 * n).astype(np.float32)        # written
    pad = 8

    def place(h, shift):
        buf = np.full(3 * n + 2 * pad, 12345.0, dtype=np.float32)
        buf[pad + shift:pad + shift + 3 * n] = h
        t = dev(buf)
        return buf, t, t[pad + shift:pad + shift + 3 * n]

    hb, tb, vb = place(b, shift_read)
    ha, ta, va = place(a, shift_write)
    assert vb.data_ptr() % 16 == 4 * (shift_read % 4) and va.data_ptr() % 16 == 4 * (shift_write % 4)
    par = dev(np.array([0.37, 0, 0, 1.2, 0.9, 1.1], dtype=np.float32))
    if op == "step":
        engine.step(va, vb, DS, n)
    elif op == "add_elastic":
        engine.add_elastic(vb, va, n, dev(k) if k is not None else None)
    elif op == "elastic":
        engine.elastic(vb, va, n, dev(k))
    elif op == "rescale":
        engine.rescale(va, n, par)
    got_a, got_b = ta.cpu().numpy(), tb.cpu().numpy()
    what = "%s n=%d read+%d write+%d" % (op, n, shift_read, shift_write)
    lo, hi = pad + shift_write, pad + shift_write + 3 * n
    exact, value = expected(op, b, a, k)
    if exact is not None:
        assert_correctly_rounded(got_a[lo:hi], exact, what)
    else:
        np.testing.assert_array_equal(got_a[lo:hi], value, err_msg=what)
    # the floats in front of the view and behind it, and everything the kernel only reads
    np.testing.assert_array_equal(got_a[:lo], ha[:lo], err_msg=what + ": written in front of the array")
    np.testing.assert_array_equal(got_a[hi:], ha[hi:], err_msg=what + ": written behind the array")
    np.testing.assert_array_equal(got_b, hb, err_msg=what + ": the input changed")


@pytest.mark.parametrize("op,k", [("step", K3), ("add_elastic", K3), ("add_elastic", None), ("elastic", K3), ("rescale", K3)],
                         ids=["step", "add_elastic", "add_elastic_null_k", "elastic", "rescale"])
def test_stream_kernels_second_grid_pass(engine, op, k):
    run_stream(engine, op, N_STREAM, seed=3, k=k)


def test_permutation_kernels_second_grid_pass(engine):
    import torch
    n = N_STREAM
    rng = np.random.default_rng(4)
    src = rng.standard_normal((n, 3)).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)
    s, m = dev(src), dev(perm)
    d = torch.full_like(s, 12345.0)
    engine.gather(d, s, m, n)                                   # dst[i] = src[map[i]]
    np.testing.assert_array_equal(d.cpu().numpy(), src[perm])
    d2 = torch.full_like(s, 12345.0)
    engine.gather_inverse(d2, s, m, n)                          # dst[map[i]] = src[i]
    want = np.empty_like(src)
    want[perm] = src
    np.testing.assert_array_equal(d2.cpu().numpy(), want)
    rep = rng.integers(0, n, n).astype(np.int32)                # a map that repeats indices (and leaves others out)
    assert len(np.unique(rep)) < n
    d3 = torch.full_like(s, 12345.0)
    engine.gather(d3, s, dev(rep), n)
    np.testing.assert_array_equal(d3.cpu().numpy(), src[rep])
    d4 = torch.full_like(s, 12345.0)
    engine.copy(d4, s, n)
    np.testing.assert_array_equal(d4.cpu().numpy(), src)
    np.testing.assert_array_equal(s.cpu().numpy(), src)


@pytest.mark.parametrize("n", [4, 1001, 200003])
def test_stream_kernels_off_alignment(engine, n):
    """views one float off 16-byte alignment (the scalar paths, which keep the component phase), and for the elastic kernels one
    pointer aligned and the other not; 200003 makes the scalar kernels loop (600009 floats > 524288 threads)"""
    for op in ("step", "add_elastic", "elastic", "rescale"):
        run_stream(engine, op, n, 1, 1, seed=n)
    run_stream(engine, "add_elastic", n, 1, 1, seed=n + 1, k=None)
    for op in ("add_elastic", "elastic", "step"):
        run_stream(engine, op, n, 1, 0, seed=n + 2)           # only p shifted
        run_stream(engine, op, n, 0, 1, seed=n + 3)           # only a shifted
    for op in ("step", "add_elastic", "elastic"):              # aligned, inside the same guards
        run_stream(engine, op, n, 0, 0, seed=n + 4)
        run_stream(engine, op, n, 3, 2, seed=n + 5)


# ---- F. integrators at a step where the constants show ------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ig.SCALES)
@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_integrators_elastic_only_against_fp64_restatement(engine, oracle32, scheme, scale):
    """a = -k o x alone (param[0] = 0 multiplies the Coulomb sum by 0), dt = 1.0, six steps: x and v against the fp64 restatement
    of the scheme, within 4 x the distance of the fp32 oracle from the same restatement (fma against mul + add), at most 1e-5.
    tests/test_integrators3d_host.py shows that a constant wrong by 1e-3 moves x or v by 30 x this tolerance or more.
    oracle32 floors: 6e-08 to 1.3e-06, by scheme and scale in that module's docstring."""
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    buf, par = ig.elastic_only_input(oracle32)
    want = ig.restated(buf, par, scheme, scale)
    floor = ig.oracle32_floor(oracle32, buf, par, scheme, scale)
    tol = ig.gpu_tolerance(floor)
    d, prm = dev(buf.copy()), dev(par)
    engine.compute_force(EVAL_DIRECT_KAHAN, d, ig.N, prm, elastic=True)
    for _ in range(ig.STEPS):
        engine.integrate(scheme, EVAL_DIRECT_KAHAN, d, ig.N, prm, ig.DT, scale, elastic=True)
    got = d.cpu().numpy()
    err = tuple(ig.rel_dist(got[k], want[k]) for k in range(2))
    print("%-10s scale %.1f: gpu x %.2e v %.2e   oracle32 x %.2e v %.2e   tolerance x %.2e v %.2e"
          % (ig.NAMES[scheme], scale, err[0], err[1], floor[0], floor[1], tol[0], tol[1]))
    assert np.isfinite(got).all()
    assert err[0] <= tol[0] and err[1] <= tol[1], (err, tol)


@pytest.mark.parametrize("elastic", [True, False], ids=["elastic", "coulomb_only"])
@pytest.mark.parametrize("scale", ig.SCALES)
@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_integrators_coulomb_against_fp64_oracle_per_step(engine, oracle32, oracle64, scheme, scale, elastic):
    """n = 512, dt = 0.02, three steps of the Coulomb (+ elastic) flow: after every step x and v within 4 x the distance of the fp32
    oracle from the fp64 oracle at that step.  This flow amplifies rounding (Forest-Ruth's negative sub-step most of all), so the
    bound can only come from the reference run; its only cap is 1e-2.  nbco_integrate_steps gives the bits of three calls.
    oracle32 against oracle64 after three steps: x 6e-08 to 7e-08 and v 6e-08 to 3e-07 for Euler, pre-Euler and leapfrog; x 2e-07,
    v 4e-07 for PEFRL; Forest-Ruth x 2e-06 to 7e-05, v 4e-05 to 6e-04."""
    import torch
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    from oracle import pyoracle as po
    n, dt, steps = 512, 0.02, 3
    buf = oracle32.init_reference(n)
    par = oracle32.params(n)
    b32, b64 = buf.copy(), buf.astype(np.float64)
    p64 = par.astype(np.float64)
    oracle32.compute_force(po.KIND_DIRECT3, b32, par, elastic=elastic, eps2=f32(1e-18))
    oracle64.compute_force(po.KIND_DIRECT3, b64, p64, elastic=elastic, eps2=f32(1e-18))
    d, prm = dev(buf.copy()), dev(par)
    engine.compute_force(EVAL_DIRECT_KAHAN, d, n, prm, elastic=elastic)
    start = d.clone()
    for s in range(steps):
        oracle32.integrate(scheme, po.KIND_DIRECT3, b32, par, dt, scale, elastic=elastic, eps2=f32(1e-18))
        oracle64.integrate(scheme, po.KIND_DIRECT3, b64, p64, dt, scale, elastic=elastic, eps2=f32(1e-18))
        engine.integrate(scheme, EVAL_DIRECT_KAHAN, d, n, prm, dt, scale, elastic=elastic)
        got = d.cpu().numpy()
        assert np.isfinite(got).all()
        floor = tuple(ig.rel_dist(b32[k], b64[k]) for k in range(2))
        err = tuple(ig.rel_dist(got[k], b64[k]) for k in range(2))
        tol = ig.gpu_tolerance(floor, cap=1e-2)
        print("%-10s scale %.1f elastic %d step %d: gpu x %.2e v %.2e   oracle32 x %.2e v %.2e"
              % (ig.NAMES[scheme], scale, elastic, s + 1, err[0], err[1], floor[0], floor[1]))
        assert err[0] <= tol[0] and err[1] <= tol[1], (s + 1, err, tol)
    engine.integrate_steps(scheme, EVAL_DIRECT_KAHAN, start, n, prm, dt, steps, scale, elastic=elastic)
    assert torch.equal(start.view(torch.int32), d.view(torch.int32)), "nbco_integrate_steps differs from three nbco_integrate calls"
