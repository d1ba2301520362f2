"""GPU parity tests of the uniform-octree evaluator with traceless multipoles (nbco_fmm_traceless, through the C ABI)
against the CPU oracle (fmm_cart3_traceless.cuh restated in oracle/nbco_oracle.cpp).

Bar: integer cell keys, the sort permutation and the cell ranges bit-exact; positions / velocities left in the
same (cell) order; expansions and accelerations within 1e-5 (nbutil.force_err) of the oracle."""
import numpy as np
import pytest

from nbutil import force_err

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def state(o, n, kind):
    if kind == "gauss":
        return o.init_reference(n)
    if kind == "cube":
        return o.init_reference(n, test_mode=True)
    rng = np.random.default_rng(99 + n)
    buf = np.zeros((3, n, 3), dtype=np.float32)
    buf[0] = rng.standard_normal((n, 3)).astype(np.float32) * np.array([1.0, 0.6, 0.3], dtype=np.float32)
    buf[1] = rng.standard_normal((n, 3)).astype(np.float32)
    return buf


def run_gpu(engine, buf, par, n, **opts):
    import torch
    engine.set(**opts)
    d = dev(buf[:2])
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    engine.fmm_cart3_traceless(d, a, n, dev(par) if par is not None else None)
    torch.cuda.synchronize()
    return d.cpu().numpy(), a.cpu().numpy()


@pytest.mark.parametrize("n,p,kind", [(4096, 6, "cube"), (4096, 6, "gauss"), (30001, 6, "blob"), (5000, 8, "cube"),
                                      (20000, 4, "blob"), (700, 3, "cube"), (65536, 7, "blob"), (8000, 10, "blob")])
def test_cells_bit_exact_and_forces(engine, oracle32, oracle64, n, p, kind):
    o = oracle32
    buf = state(o, n, kind)
    par = o.params(n)
    pv, want = o.fmm_oct_traceless(buf[:2], par, p=p, threads=8)
    tree = o.oct_tree(n)
    ex = o.oct_expansions(p)
    got_pv, got = run_gpu(engine, buf, par, n, fmm_order=p)
    info = engine.oct_info()
    assert (info.L, info.ntot, info.order, info.n) == (tree["L"], tree["ntot"], p, n)
    np.testing.assert_array_equal(engine.oct_array("keys").astype(np.int64), tree["keys"])
    np.testing.assert_array_equal(engine.oct_array("perm").astype(np.int64), tree["perm"])
    beg = ((1 << (3 * info.L)) - 1) // 7
    np.testing.assert_array_equal(engine.oct_array("index")[beg:], tree["index"][beg:])
    first = 9    # levels 0 and 1 carry nothing
    np.testing.assert_array_equal(engine.oct_array("mult")[first:], tree["mult"][first:])
    # state left in cell order, bit for bit
    np.testing.assert_array_equal(got_pv, pv)
    assert force_err(got, want) < 1e-5
    # centres and expansions.  A cell of a clustered input holds thousands of particles and the P2M sums run in a
    # different order (wave-strided partial sums here, one sequential fp32 sum in the oracle): the yardstick for the
    # raw tuples is the fp64 oracle, against which the GPU must be as good as the fp32 oracle is.
    c4 = engine.oct_array("center4")
    scale = np.abs(ex["center"][first:]).max() + 1e-30
    assert np.abs(c4[first:, :3] - ex["center"][first:]).max() / scale < 1e-6
    occupied = tree["mult"][first:] > 0    # the oracle also pushes locals into empty cells; nobody reads them
    o64 = oracle64
    o64.fmm_oct_traceless(buf[:2].astype(np.float64), par.astype(np.float64), p=p, threads=8)
    same_cells = np.array_equal(o64.oct_tree(n)["keys"], tree["keys"])
    ex64 = o64.oct_expansions(p)
    for name in ("mpole", "local"):
        g, w = engine.oct_array(name)[first:][occupied], ex[name][first:][occupied]
        sc = np.abs(w).max(axis=0, keepdims=True).clip(1e-30)
        err = (np.abs(g - w) / sc).max()
        if same_cells:
            t = ex64[name][first:][occupied]
            floor = (np.abs(w - t) / sc).max()
            assert (np.abs(g - t) / sc).max() < 2 * floor + 2e-5, name
        else:
            assert err < 1e-3, name


@pytest.mark.parametrize("p", [1, 2, 5])
def test_low_orders(engine, oracle32, p):
    """orders below 6: the reference's unrolled M2L contracts nothing; oracle and GPU implement the intent"""
    o = oracle32
    n = 3000
    buf = state(o, n, "blob")
    par = o.params(n)
    _, want = o.fmm_oct_traceless(buf[:2], par, p=p, threads=8)
    _, got = run_gpu(engine, buf, par, n, fmm_order=p)
    assert force_err(got, want) < 1e-5


def test_accuracy_against_direct_sum(engine, oracle32):
    """the evaluator reproduces the reference's own accuracy (2.6e-4 mean relative error at
    p = 6, N = 4096, the default Gaussian ball; same bound as tests/test_oracle_pins.py)"""
    o = oracle32
    n = 4096
    buf = state(o, n, "gauss")
    par = o.params(n)
    got_pv, got = run_gpu(engine, buf, par, n, fmm_order=6)
    ref = o.direct3(got_pv[0], par, threads=8)
    assert o.mean_relerr(got, ref) < 8e-4


def test_options_and_edges(engine, oracle32):
    o = oracle32
    # no collisions: far field only
    n = 6000
    buf = state(o, n, "blob")
    par = o.params(n)
    _, want = o.fmm_oct_traceless(buf[:2], par, p=6, threads=8, coll=False)
    _, got = run_gpu(engine, buf, par, n, fmm_order=6, coll=0)
    assert force_err(got, want) < 1e-5
    # wider stencil
    _, want = o.fmm_oct_traceless(buf[:2], par, p=6, threads=8, radius=2.0)
    _, got = run_gpu(engine, buf, par, n, fmm_order=6, coll=1, tree_radius=2.0)
    assert force_err(got, want) < 1e-5
    # inhomogeneity factor raises the level count
    _, want = o.fmm_oct_traceless(buf[:2], par, p=6, threads=8, dens_inhom=8.0)
    _, got = run_gpu(engine, buf, par, n, fmm_order=6, tree_radius=1.0, dens_inhom=8.0)
    assert engine.oct_info().L == o.oct_tree(n)["L"]
    assert force_err(got, want) < 1e-5
    engine.set(dens_inhom=1.0)
    # tiny systems (two levels is the minimum), no rescale parameter
    for n in (1, 2, 37):
        buf = state(o, n, "blob")
        _, want = o.fmm_oct_traceless(buf[:2], None, p=6, threads=1)
        _, got = run_gpu(engine, buf, None, n, fmm_order=6)
        assert np.isfinite(got).all()
        assert force_err(got, want) < 1e-5
    # coincident particles all land in one cell (softened self interactions, no NaN)
    n = 300
    buf = np.zeros((3, n, 3), dtype=np.float32)
    buf[0, :, :] = 0.25
    buf[0, :5] = np.arange(15, dtype=np.float32).reshape(5, 3)
    _, want = o.fmm_oct_traceless(buf[:2], None, p=6, threads=1, eps2=1e-4)
    _, got = run_gpu(engine, buf, None, n, fmm_order=6, eps2=1e-4)
    assert np.isfinite(got).all()
    assert force_err(got, want) < 1e-5
    engine.set(eps2=1e-18)


def test_orders_nine_and_ten(engine, oracle32):
    """BASELINE config 5 runs the traceless evaluator at p = 10; orders above 10 are rejected by the options check"""
    from coulomb_oscillators_amd import EngineError
    o = oracle32
    n = 4096
    buf = state(o, n, "cube")
    par = o.params(n)
    for p in (9, 10):
        _, want = o.fmm_oct_traceless(buf[:2], par, p=p, threads=8)
        _, got = run_gpu(engine, buf, par, n, fmm_order=p)
        assert force_err(got, want) < 1e-5
    with pytest.raises(EngineError):
        engine.set(fmm_order=11)


def test_integrate_with_octree_evaluator(engine, oracle32):
    """leapfrog through nbco_integrate with the octree evaluator against the oracle's integrator"""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_TRACELESS, INTEG_LEAPFROG
    from oracle import pyoracle as po
    o = oracle32
    n, p, dt = 4096, 6, 1e-3
    buf = state(o, n, "cube")
    par = o.params(n)
    ref = buf.copy()
    o.compute_force(po.KIND_FMM_OCT, ref, par, p=p, threads=8)
    for _ in range(3):
        o.integrate(po.SCHEME_LEAPFROG, po.KIND_FMM_OCT, ref, par, dt, p=p, threads=8)
    engine.set(fmm_order=p)
    d = dev(buf)
    prm = dev(par)
    engine.compute_force(EVAL_FMM_TRACELESS, d, n, prm)
    for _ in range(3):
        engine.integrate(INTEG_LEAPFROG, EVAL_FMM_TRACELESS, d, n, prm, dt)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    # the cell order may differ after several steps only if a particle sits within rounding of a cell face; compare as sets
    key = lambda x: np.lexsort((x[:, 2], x[:, 1], x[:, 0]))
    ka, kb = key(got[0]), key(ref[0])
    np.testing.assert_allclose(got[0][ka], ref[0][kb], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[1][ka], ref[1][kb], rtol=1e-4, atol=1e-6)


# ---- fp64 far field (opts.far_fp64; BASELINE config 5: fp64 far field / fp32 P2P) ---------------------------------
@pytest.mark.parametrize("n,p,kind", [(20000, 6, "blob"), (8000, 10, "blob"), (4096, 10, "gauss"), (3000, 3, "cube")])
def test_far_fp64_against_double_oracle(engine, oracle32, oracle64, n, p, kind):
    """expansions kept and shifted in double: the yardstick is the oracle built with SCAL = double, run on the same
    (fp32-valued) positions.  Cell centres stay fp32 here, so the tuples agree to fp32 centre rounding, not to 1e-15."""
    o, o64 = oracle32, oracle64
    buf = state(o, n, kind)
    par = o.params(n)
    pv64, want64 = o64.fmm_oct_traceless(buf[:2].astype(np.float64), par.astype(np.float64), p=p, threads=8)
    tree64 = o64.oct_tree(n)
    ex64 = o64.oct_expansions(p)
    got_pv, got = run_gpu(engine, buf, par, n, fmm_order=p, far_fp64=1)
    info = engine.oct_info()
    assert info.real_bytes == 8
    mp, lc = engine.oct_array("mpole"), engine.oct_array("local")
    assert mp.dtype == np.float64 and lc.dtype == np.float64
    same_cells = np.array_equal(engine.oct_array("keys").astype(np.int64), tree64["keys"])
    _, got32 = run_gpu(engine, buf, par, n, fmm_order=p, far_fp64=0)
    assert engine.oct_info().real_bytes == 4
    engine.set(far_fp64=0)
    if not same_cells:
        pytest.skip("a particle sits within fp32 rounding of a cell face: the double oracle bins it differently")
    np.testing.assert_array_equal(got_pv, pv64.astype(np.float32))
    e64, e32 = force_err(got, want64), force_err(got32, want64)
    assert e64 < 1e-5
    assert e64 < 1.5 * e32 + 2e-7          # never worse than the all-fp32 evaluation
    first = 9
    occupied = tree64["mult"][first:] > 0
    for name, g in (("mpole", mp), ("local", lc)):
        w = ex64[name][first:][occupied]
        sc = np.abs(w).max(axis=0, keepdims=True).clip(1e-300)
        assert (np.abs(g[first:][occupied] - w) / sc).max() < 2e-5, name


def test_far_fp64_keeps_high_orders_in_range(engine, oracle32):
    """p = 10 on the BASELINE Gaussian ball with six octree levels (config 5 has seven): the fp32 far field leaves its
    range (r^-11 19!! ~ 1e40, SURVEY N8: NaN / inf in the result), the fp64 far field stays finite and follows the
    direct sum.  With the reference's default stencil radius 1 the error is truncation-bound (3e-4, the same in both
    precisions wherever fp32 survives); radius 2 shows what is left: 1.5e-5, the fp32 near field."""
    import torch
    o = oracle32
    n, p = 1 << 20, 10
    buf = state(o, n, "gauss")
    par = o.params(n)
    prm = dev(par)
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    ref = torch.zeros_like(a)
    for radius, bound in ((1.0, 6e-4), (2.0, 4e-5)):
        d = dev(buf[:2])
        engine.set(fmm_order=p, far_fp64=1, dens_inhom=4.0, tree_radius=radius)
        engine.fmm_cart3_traceless(d, a, n, prm)
        torch.cuda.synchronize()
        assert engine.oct_info().L == 6
        assert bool(torch.isfinite(a).all())
        engine.direct(d, ref, n, prm)          # d is now in cell order; the direct sum runs on the same order
        torch.cuda.synchronize()
        err = engine.mean_relerr(a, ref, n)
        assert err < bound, (radius, err)
    # the all-fp32 evaluation of the same system overflows
    d32 = dev(buf[:2])
    engine.set(far_fp64=0, tree_radius=1.0)
    engine.fmm_cart3_traceless(d32, a, n, prm)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(a).all())
    engine.set(dens_inhom=1.0)


# ---- the octree evaluator with SYMMETRIC multipoles, `fmm_cart3` (fmm_cart3_symmetric.cuh:413-580) ----------------------------
@pytest.mark.parametrize("n,p,kind", [(4096, 6, "cube"), (4096, 6, "gauss"), (30001, 5, "blob"), (5000, 8, "cube"), (20000, 4, "blob"),
                                      (700, 3, "cube"), (3000, 1, "blob"), (3000, 2, "blob"), (8000, 9, "blob")])
def test_symmetric_evaluator_matches_oracle(engine, oracle32, oracle64, n, p, kind):
    """nbco_fmm_symmetric: same cells, same sort, same stencils as the traceless evaluator; symmetric multipole tuples of orders
    0..p (compared with the oracle's fmm_cart3_cpu restatement), accelerations within 1e-5"""
    import torch
    o = oracle32
    buf = state(o, n, kind)
    par = o.params(n)
    pv, want = o.fmm_oct_symmetric(buf[:2], par, p=p, threads=8)
    tree = o.oct_tree(n)
    ex = o.oct_expansions(p, symmetric=True)
    engine.set(fmm_order=p)
    d = dev(buf[:2])
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    engine.fmm_cart3(d, a, n, dev(par))
    torch.cuda.synchronize()
    info = engine.oct_info()
    assert info.mpole_reals == (p + 1) * (p + 2) * (p + 3) // 6
    np.testing.assert_array_equal(engine.oct_array("keys").astype(np.int64), tree["keys"])
    np.testing.assert_array_equal(engine.oct_array("perm").astype(np.int64), tree["perm"])
    np.testing.assert_array_equal(d.cpu().numpy(), pv)
    assert force_err(a.cpu().numpy(), want) < 1e-5
    # multipole and local tuples against the fp64 oracle: as good as the fp32 oracle is
    first = 9
    occupied = tree["mult"][first:] > 0
    oracle64.fmm_oct_symmetric(buf[:2].astype(np.float64), par.astype(np.float64), p=p, threads=8)
    if np.array_equal(oracle64.oct_tree(n)["keys"], tree["keys"]):
        ex64 = oracle64.oct_expansions(p, symmetric=True)
        for name in ("mpole", "local"):
            g, w, t = (x[name][first:][occupied] for x in ({"mpole": engine.oct_array("mpole"), "local": engine.oct_array("local")}, ex, ex64))
            sc = np.abs(t).max(axis=0, keepdims=True).clip(1e-30)
            floor = (np.abs(w - t) / sc).max()
            assert (np.abs(g - t) / sc).max() < 2 * floor + 2e-5, name


def test_symmetric_and_traceless_evaluators_agree(engine, oracle32):
    """contracting with the (traceless) gradient of 1/r only sees the traceless part of a multipole: both octree evaluators
    describe the same far field, and reach the direct sum equally well at an order where the reference's traceless M2M is exact"""
    import torch
    o = oracle32
    n, p = 20000, 8
    buf = state(o, n, "blob")
    par = dev(o.params(n))
    engine.set(fmm_order=p)
    d1, d2 = dev(buf[:2]), dev(buf[:2])
    a1 = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    a2 = torch.zeros_like(a1)
    engine.fmm_cart3_traceless(d1, a1, n, par)
    engine.fmm_cart3(d2, a2, n, par)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2)
    ref = o.direct3(d1[0].cpu().numpy(), o.params(n), threads=8)
    e1, e2 = o.mean_relerr(a1.cpu().numpy(), ref), o.mean_relerr(a2.cpu().numpy(), ref)
    assert e2 < 1.05 * e1 + 1e-6 and e2 < 3e-4
    # order 10 has no generated symmetric operators (they come from the order p + 1 kd-tree set)
    from coulomb_oscillators_amd import EngineError
    engine.set(fmm_order=10)
    with pytest.raises(EngineError, match="orders 1..9"):
        engine.fmm_cart3(d2, a2, n, par)


def test_baseline_config_2_by_name_properties(engine, oracle32):
    """BASELINE configs[2] by name -- "FMM-3D cartesian traceless p=6, N=1M, 1xMI355X" -- at its own size, where the oracle takes
    too long to be the checker: the sorted cell keys against the key formula itself (appel.cuh:44-55: row-major
    flatten of the clipped integer cell coordinates, fp32, no contraction) in numpy, bit for bit; the permutation is one and
    carries the state; every acceleration finite; and the accelerations of a sample of particles against an fp64 direct sum
    over all 2^20 sources.  On this input (anisotropic ball in a cubic grid) the octree is an almost all-pairs run: ~600 of
    32 768 leaf cells are occupied, so the far field carries little and the result is close to the direct sum."""
    import torch
    o = oracle32
    n, p = 1 << 20, 6
    buf = state(o, n, "gauss")
    par = o.params(n)
    got_pv, got = run_gpu(engine, buf, par, n, fmm_order=p, far_fp64=0, dens_inhom=1.0, tree_radius=1.0)
    info = engine.oct_info()
    assert (info.order, info.n, info.real_bytes) == (p, n, 4)
    assert np.isfinite(got).all() and np.isfinite(got_pv).all()
    # T1 in numpy (float32 throughout; (x - min) * rdelta is one subtraction and one multiplication, truncated towards zero)
    L, side = info.L, 1 << info.L
    pos = buf[0]
    mn, mx = pos.min(0), pos.max(0)
    delta = np.float32((mx - mn).max()) / np.float32(side)
    eps = np.sqrt(np.float32(engine.opts().eps2))
    delta = max(delta, eps)
    rdelta = np.float32(1) / np.float32(delta)
    q = ((pos - mn) * rdelta).astype(np.float32)
    ijk = np.clip(q.astype(np.int32), 0, side - 1).astype(np.int64)
    keys = (ijk[:, 0] * side + ijk[:, 1]) * side + ijk[:, 2]
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(engine.oct_array("keys").astype(np.int64), keys[order])
    np.testing.assert_array_equal(engine.oct_array("perm").astype(np.int64), order)
    np.testing.assert_array_equal(got_pv[0], pos[order])
    np.testing.assert_array_equal(got_pv[1], buf[1][order])
    # (SURVEY's numpy estimate for a ball of this shape was 625 occupied cells of 32 768; the reference's own stream gives 588)
    assert L == 5 and 400 < len(np.unique(keys)) < 800
    # sampled fp64 direct sum (the evaluator's convention: a_i = param[0] sum_j (x_i - x_j) / (|x_i - x_j|^2 + eps2)^(3/2))
    rng = np.random.default_rng(11)
    pick = rng.choice(n, 192, replace=False)
    P64 = got_pv[0].astype(np.float64)
    eps2 = float(engine.opts().eps2)
    want = np.empty((len(pick), 3))
    for k, i in enumerate(pick):
        d = P64[i] - P64
        r2 = (d * d).sum(1) + eps2
        w = r2 ** -1.5
        w[i] = 0.0
        want[k] = float(par[0]) * (d * w[:, None]).sum(0)
    mag = np.linalg.norm(want, axis=1)
    err = np.linalg.norm(got[pick] - want, axis=1) / (mag + np.abs(mag).mean())
    # stencil radius 1 at p = 6: truncation-bound, the level the reference's own -test table records (8.7e-3 at p = 6 on a
    # cube); the near field here covers almost everything
    assert err.max() < 2e-3, err.max()


# ---- every accepted (evaluator, precision, order): the order is chosen per kernel launch, once per kernel ----------------------
ORDER_SWEEP = [(ev, f64, p) for ev, top in (("traceless", 10), ("symmetric", 9)) for f64 in (0, 1) for p in range(1, top + 1)]


@pytest.mark.parametrize("evaluator,far_fp64,p", ORDER_SWEEP)
def test_every_order_reaches_its_own_kernels(engine, oracle32, oracle64, evaluator, far_fp64, p):
    """A wrong case label in the order dispatch gives a plausible but less accurate force, or tuples of another order's size.
    n = 3000 on the blob: L = 2..4 over the orders, so M2M, M2L, L2L and a near field of several cells all run.  The bars are
    this file's: test_low_orders / test_orders_nine_and_ten (traceless), test_symmetric_evaluator_matches_oracle (symmetric)
    and test_far_fp64_against_double_oracle (far_fp64, each evaluator against its own SCAL = double oracle)."""
    import torch
    n = 3000
    sym = evaluator == "symmetric"
    buf = state(oracle32, n, "blob")
    par = oracle32.params(n)

    def gpu(f64):
        engine.set(fmm_order=p, far_fp64=f64)
        d = dev(buf[:2])
        a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        (engine.fmm_cart3 if sym else engine.fmm_cart3_traceless)(d, a, n, dev(par))
        torch.cuda.synchronize()
        return d.cpu().numpy(), a.cpu().numpy()

    o = oracle64 if far_fp64 else oracle32
    real = np.float64 if far_fp64 else np.float32
    pv, want = (o.fmm_oct_symmetric if sym else o.fmm_oct_traceless)(buf[:2].astype(real), par.astype(real), p=p, threads=8)
    tree = o.oct_tree(n)
    got_pv, got = gpu(far_fp64)
    info = engine.oct_info()
    reals = (p + 1) * (p + 2) * (p + 3) // 6 if sym else (p + 1) ** 2
    mp = engine.oct_array("mpole")
    assert (info.order, info.L, info.ntot, info.real_bytes) == (p, tree["L"], tree["ntot"], 8 if far_fp64 else 4)
    assert 2 <= info.L <= 4
    assert info.mpole_reals == reals and mp.size == info.ntot * reals and mp.dtype == real
    np.testing.assert_array_equal(engine.oct_array("keys").astype(np.int64), tree["keys"])
    np.testing.assert_array_equal(got_pv, pv.astype(np.float32))
    err = force_err(got, want)
    print("oct %s far_fp64=%d p=%d L=%d err=%.3e" % (evaluator, far_fp64, p, info.L, err))
    assert err < 1e-5
    if far_fp64:
        _, got32 = gpu(0)
        assert engine.oct_info().real_bytes == 4
        e32 = force_err(got32, want)
        print("oct %s p=%d all-fp32 against the double oracle err=%.3e" % (evaluator, p, e32))
        assert err < 1.5 * e32 + 2e-7          # never worse than the all-fp32 evaluation
    engine.set(far_fp64=0)
