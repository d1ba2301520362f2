"""GPU parity tests of the three 3-D tree evaluators on the inputs of shapes3d.CASES -- flat, collinear, tied, duplicated, offset and
late-run states -- against the two CPU oracles.  test_shapes3d_host.py shows, without a GPU, that the oracles are sound on every
"forces" case and that each bound used here tells a wrong evaluation from a right one.

Bounds, with floor = force_err(oracle32, oracle64) of the case (shapes3d.force_bound):
    force_err(gpu, oracle32) < max(1e-5, 4 floor)         force_err(gpu, oracle64) < max(1e-5, 4 floor) + floor
Trees, keys, permutations and lists are compared bit for bit on EVERY case, also where the reference's forces mean nothing.
Every measured figure is printed (run with -s)."""
import numpy as np
import pytest

import shapes3d as S
from nbutil import assert_same_tree, canon_pairs, directed_pairs, expansion_err, force_err

pytestmark = pytest.mark.gpu

KD = [c for c in S.CASES if c[0] == "kd"]
OCT = [c for c in S.CASES if c[0] != "kd"]
KD_OPTIONS = [("kd", "late", 4096, 4, "forces"), ("kd", "dup8", 4096, 4, "forces"), ("kd", "plane", 4096, 4, "forces"),
              ("kd", "late", 8000, 6, "forces")]
assert set(KD_OPTIONS) <= set(KD)
_direct = {}


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_kd(engine, buf, par, n, **opts):
    import torch
    engine.set(**opts)
    d = dev(buf[:2])
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    engine.fmm_cart3_kdtree(d, a, n, dev(par))
    torch.cuda.synchronize()
    return d.cpu().numpy(), a.cpu().numpy()


def run_oct(engine, ev, buf, par, n, **opts):
    import torch
    engine.set(**opts)
    d = dev(buf[:2])
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    (engine.fmm_cart3 if ev == "symmetric" else engine.fmm_cart3_traceless)(d, a, n, dev(par))
    torch.cuda.synchronize()
    return d.cpu().numpy(), a.cpu().numpy()


def direct64(oracle64, case, r):
    """the fp64 direct sum of a case, once per process"""
    if case not in _direct:
        _direct[case] = oracle64.direct3(r["buf"][0].astype(np.float64), r["par"].astype(np.float64), threads=S.THREADS)
    return _direct[case]


def assert_forces(tag, got, r):
    """the two force bounds of a "forces" case whose fp32 oracle is finite; prints what it measures"""
    e32, e64 = force_err(got, r["a32"]), force_err(got, r["a64"])
    bound = S.force_bound(r["floor"])
    print("%s: gpu-oracle32 %.3e gpu-oracle64 %.3e floor %.3e bound %.3e" % (tag, e32, e64, r["floor"], bound))
    assert e32 < bound
    assert e64 < bound + r["floor"]


# ---- kd-tree ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KD, ids=S.case_id)
def test_kdtree_tree_lists_and_forces(engine, oracle32, oracle64, case):
    """Every case: the tree (index, mult, splitdim, bounds, centres), the permutation, both lists as sets and the directed pair
    count are the fp32 oracle's, bit for bit, whatever way the build took (build_mode is printed: ties and zero extents may send it
    to the three-pass select or to the sorting build).  "forces" cases: accelerations within the two bounds, the same convergence to
    the fp64 direct sum as the oracle's, multipoles and locals as close to the fp32 oracle as two fp32 evaluations can be (over the
    columns that mean something in fp32, shapes3d.alive_columns: on plane_off and the lattice the moments that vanish by symmetry
    are rounding noise in BOTH oracles, 1e290 of the column's scale apart)."""
    _, shape, n, p, what = case
    r = S.evaluate(oracle32, oracle64, case)
    pv, a = run_kd(engine, r["buf"], r["par"], n, fmm_order=p, unsort=1)
    info = engine.kd_info()
    print("%s: build_mode %d, %d leaf pairs, %d M2L pairs" % (S.case_id(case), info.build_mode, info.p2p_pairs, info.m2l_pairs))
    assert_same_tree(engine, r["t32"], n, r["t32"]["perm"])
    np.testing.assert_array_equal(pv, r["buf"][:2])
    if what != "forces":
        if r["finite32"]:
            print("%s (no assertion): gpu-oracle32 %.3e gpu-oracle64 %.3e floor %.3e" % (S.case_id(case), force_err(a, r["a32"]),
                                                                                     force_err(a, r["a64"]), r["floor"]))
        return
    assert_forces(S.case_id(case), a, r)
    ref = direct64(oracle64, case, r)
    mre_gpu, mre_o32 = oracle64.mean_relerr(a, ref), oracle64.mean_relerr(r["a32"], ref)
    print("%s: mean relative error against the fp64 direct sum: gpu %.4e oracle32 %.4e" % (S.case_id(case), mre_gpu, mre_o32))
    assert abs(mre_gpu - mre_o32) <= 0.02 * mre_o32 + 2e-6
    for name in ("mpole", "local"):
        alive = S.alive_columns(r["t32"][name], r["t64"][name])
        err = S.column_errs(engine.kd_array(name), r["t32"][name])[alive].max()
        floor = S.column_errs(r["t32"][name], r["t64"][name])[alive].max()
        print("%s: %s gpu-oracle32 %.3e, oracle32-oracle64 %.3e (%d of %d columns)" % (S.case_id(case), name, err, floor, alive.sum(), len(alive)))
        assert err < 2 * floor + 2e-5, name


def test_a_non_finite_evaluation_poisons_nothing(oracle32, oracle64):
    """dup64 gives NaN in the reference and need not be finite here; the Gaussian ball evaluated afterwards on the same context is
    bit-identical to its evaluation on a fresh context: nothing non-finite survives in the context's buffers, hints or lists"""
    from coulomb_oscillators_amd import Engine
    bad = S.evaluate(oracle32, oracle64, ("kd", "dup64", 4096, 4, "lists"))
    good = S.evaluate(oracle32, oracle64, ("kd", "gauss", 4096, 4, "forces"))
    n, p = 4096, 4
    used, fresh = Engine(), Engine()
    _, a_bad = run_kd(used, bad["buf"], bad["par"], n, fmm_order=p, unsort=1)
    print("dup64 on the GPU: %d of %d accelerations finite" % (np.isfinite(a_bad).all(axis=1).sum(), n))
    assert_same_tree(used, bad["t32"], n, bad["t32"]["perm"])
    _, a_used = run_kd(used, good["buf"], good["par"], n, fmm_order=p, unsort=1)
    assert_same_tree(used, good["t32"], n, good["t32"]["perm"])
    _, a_fresh = run_kd(fresh, good["buf"], good["par"], n, fmm_order=p, unsort=1)
    np.testing.assert_array_equal(a_used, a_fresh)
    for name in ("mpole", "local"):
        np.testing.assert_array_equal(used.kd_array(name), fresh.kd_array(name))
    assert_forces("gauss after dup64", a_used, good)
    used.close(); fresh.close()


@pytest.mark.parametrize("case", KD_OPTIONS, ids=S.case_id)
def test_kdtree_options(engine, oracle32, oracle64, case):
    """unsort, m2l_first and p2p_mutual on the long-list, duplicated and flat inputs, each against the fp32 oracle run with the same
    option and under the case's own bound"""
    _, shape, n, p, _ = case
    r = S.evaluate(oracle32, oracle64, case)
    buf, par = r["buf"], r["par"]
    bound = S.force_bound(r["floor"])
    tag = S.case_id(case)
    # unsort = 0: the state comes back in the oracle's tree order
    a_t, pv_t, t_t = S.run_oracle(oracle32, "kd", buf, par, p, expansions=False, unsort=False)
    pv, a = run_kd(engine, buf, par, n, fmm_order=p, unsort=0)
    np.testing.assert_array_equal(pv, pv_t)
    assert_same_tree(engine, t_t, n, t_t["perm"])
    e = force_err(a, a_t)
    print("%s unsort=0: gpu-oracle32 %.3e bound %.3e" % (tag, e, bound))
    assert e < bound
    # m2l_first: the GPU reference's traversal order
    a_m, _, t_m = S.run_oracle(oracle32, "kd", buf, par, p, expansions=False, m2l_first=1)
    assert np.isfinite(a_m).all()
    for flag, want_a, want_t in ((1, a_m, t_m), (0, r["a32"], r["t32"])):
        _, a = run_kd(engine, buf, par, n, fmm_order=p, unsort=1, m2l_first=flag)
        assert_same_tree(engine, want_t, n, want_t["perm"])
        e = force_err(a, want_a)
        print("%s m2l_first=%d: gpu-oracle32 %.3e bound %.3e, %d + %d list entries" % (tag, flag, e, bound, len(want_t["p2p"]), len(want_t["m2l"])))
        assert e < bound
    # p2p_mutual: Newton's third law per leaf pair; same lists, same bound, reproducible
    _, a_one = run_kd(engine, buf, par, n, fmm_order=p, unsort=1, p2p_mutual=0)
    assert engine.kd_info().p2p_halves == 0
    _, a_mut = run_kd(engine, buf, par, n, fmm_order=p, unsort=1, p2p_mutual=1)
    halves = engine.kd_info().p2p_halves
    assert_same_tree(engine, r["t32"], n, r["t32"]["perm"])
    _, a_mut2 = run_kd(engine, buf, par, n, fmm_order=p, unsort=1, p2p_mutual=1)
    print("%s p2p_mutual: halves %d, one-directional %.3e mutual %.3e bound %.3e" % (tag, halves, force_err(a_one, r["a32"]), force_err(a_mut, r["a32"]), bound))
    assert force_err(a_one, r["a32"]) < bound and force_err(a_mut, r["a32"]) < bound
    np.testing.assert_array_equal(a_mut, a_mut2)
    # leaves of 31 / 32 particles are taken as one half each; the 16-particle leaves of (4096, 4) fill the rows too badly and run
    # the one-directional kernel (test_mutual_near_field_matches_oracle_and_the_one_directional_kernel)
    assert halves == (1 if n == 8000 else 0)


@pytest.mark.parametrize("case", KD_OPTIONS + [("kd", "line", 4096, 10, "lists")], ids=S.case_id)
def test_kdtree_far_fp64(engine, oracle32, oracle64, case):
    """far_fp64 = 1: geometry and lists unchanged, bit for bit; never further from the fp64 oracle than the all-fp32 evaluation is
    (the rule of test_far_fp64_kdtree_against_both_oracles).  A line at p = 10 leaves the fp32 range in the reference; there the fp64
    far field has to be finite and within 1e-5 of the fp64 oracle, and nothing is asked of the fp32 run."""
    _, shape, n, p, _ = case
    r = S.evaluate(oracle32, oracle64, case)
    assert S.same_kd_lists(r["t32"], r["t64"])
    _, got32 = run_kd(engine, r["buf"], r["par"], n, fmm_order=p, unsort=1, far_fp64=0)
    assert engine.kd_info().real_bytes == 4
    _, got = run_kd(engine, r["buf"], r["par"], n, fmm_order=p, unsort=1, far_fp64=1)
    assert engine.kd_info().real_bytes == 8
    assert_same_tree(engine, r["t32"], n, r["t32"]["perm"])
    mp, lc = engine.kd_array("mpole"), engine.kd_array("local")
    assert mp.dtype == np.float64 and lc.dtype == np.float64
    assert np.isfinite(got).all() and np.isfinite(mp).all() and np.isfinite(lc).all()
    e64 = force_err(got, r["a64"])
    if r["finite32"]:
        e32 = force_err(got32, r["a64"])
        print("%s far_fp64: gpu64-oracle64 %.3e gpu32-oracle64 %.3e floor %.3e" % (S.case_id(case), e64, e32, r["floor"]))
        assert e64 <= 1.5 * e32 + 2e-7
        assert e64 < S.force_bound(r["floor"]) + r["floor"]
    else:
        print("%s far_fp64: gpu64-oracle64 %.3e (fp32 oracle not finite; fp32 GPU run: %d of %d finite)"
              % (S.case_id(case), e64, np.isfinite(got32).all(axis=1).sum(), n))
        assert e64 < 1e-5
    for name, g in (("mpole", mp), ("local", lc)):
        err = expansion_err(g, r["t64"][name])
        print("%s far_fp64: %s gpu64-oracle64 %.3e" % (S.case_id(case), name, err))
        assert err < (2e-5 if p <= 6 else 1e-4), name          # the rounding of the fp32 centres, seen k times by a term of order k


@pytest.mark.parametrize("mutual", [0, 1])
def test_long_range_kernel_against_the_oracle(oracle32, oracle64, mutual):
    """The late-run state of test_long_ranges_take_their_own_kernel_when_the_lists_are_long (65536 particles, three of them far
    away, opening radius 2: per-target ranges of thousands of entries), three evaluations on one context.  That test compares the
    evaluations with each other; here the first (radix path) and the second (long_lists = 1: ranges above 512 entries sorted by
    list_longsort_kernel) are each compared with the fp32 oracle run on the same input: state in the oracle's tree order bit for bit,
    lists as sets, directed pair count, accelerations within the bound.  floor is the (8000, 6) late case's: the fp64 oracle and the
    fp64 direct sum are not run at this size."""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, Engine
    n, p, radius = S.LONG_RANGE["n"], S.LONG_RANGE["p"], S.LONG_RANGE["radius"]
    floor = S.evaluate(oracle32, oracle64, S.FLOOR_CASE_OF_LONG_RANGE + ("forces",))["floor"]
    bound = S.force_bound(floor)
    first, second = S.long_range_oracle(oracle32), S.long_range_oracle(oracle32, again=True)
    par = dev(first[1])
    eng = Engine(fmm_order=p, unsort=0, tree_steps=1, tree_radius=radius, p2p_mutual=mutual)
    d = dev(first[0])
    longs = []
    for k, (buf, _, pv, a, t) in enumerate((first, second, second)):
        np.testing.assert_array_equal(d[:2].cpu().numpy(), buf[:2])          # what this evaluation is given is what the oracle was given
        eng.compute_force(EVAL_FMM_KDTREE, d, n, par, elastic=False)
        torch.cuda.synchronize()
        info = eng.kd_info()
        longs.append(info.long_lists)
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[:2], pv)
        assert (info.L, info.ntot) == (t["L"], t["ntot"])
        for name in ("p2p", "m2l"):
            np.testing.assert_array_equal(canon_pairs(eng.kd_array(name)), canon_pairs(t[name]), err_msg=name)
        assert info.directed_p2p == directed_pairs(t["mult"], t["p2p"], t["L"])
        e = force_err(got[2], a)
        print("late 65536 p2p_mutual=%d evaluation %d: long_lists %d halves %d, %d leaf pairs, gpu-oracle32 %.3e bound %.3e"
              % (mutual, k, info.long_lists, info.p2p_halves, info.p2p_pairs, e, bound))
        assert np.isfinite(got).all()
        assert e < bound
    assert longs == [0, 1, 1]
    eng.close()


# ---- octree, both evaluators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OCT, ids=S.case_id)
def test_octree_cells_and_forces(engine, oracle32, oracle64, case):
    """Every case: sorted keys, permutation, leaf ranges and multiplicities are the fp32 oracle's and the state is left in its cell
    order, bit for bit; the centroids of the occupied cells are as close to the fp64 oracle's as fp32 sums get.  "forces" cases where
    the fp32 oracle is finite: accelerations within the two bounds, expansions of the occupied cells as close to the fp64 oracle as
    the fp32 oracle's are (2 floor + 2e-5, over the columns that mean something in fp32: shapes3d.alive_columns).  Where the fp32
    oracle overflows (shapes3d.OCT_FP32_OVERFLOWS: a stretched tree) the run is far_fp64 = 1: every acceleration finite and within
    1e-5 of the fp64 oracle, the bound of test_far_fp64_against_double_oracle, and the locals of the occupied cells within that
    test's 2e-5 of the fp64 oracle's; nothing is asked of the fp32 evaluation there."""
    ev, shape, n, _, what = case
    p = S.order_of(case)
    sym = ev == "symmetric"
    r = S.evaluate(oracle32, oracle64, case)
    overflow = case[:4] in S.OCT_FP32_OVERFLOWS
    assert r["finite32"] == (not overflow)
    pv, a = run_oct(engine, ev, r["buf"], r["par"], n, fmm_order=p, far_fp64=int(overflow))
    info = engine.oct_info()
    t = r["t32"]
    assert (info.L, info.ntot, info.order, info.n, info.real_bytes) == (t["L"], t["ntot"], p, n, 8 if overflow else 4)
    assert info.mpole_reals == ((p + 1) * (p + 2) * (p + 3) // 6 if sym else (p + 1) ** 2)
    np.testing.assert_array_equal(engine.oct_array("keys").astype(np.int64), t["keys"])
    np.testing.assert_array_equal(engine.oct_array("perm").astype(np.int64), t["perm"])
    beg = ((1 << (3 * info.L)) - 1) // 7
    first = 9          # levels 0 and 1 carry nothing
    np.testing.assert_array_equal(engine.oct_array("index")[beg:], t["index"][beg:])
    np.testing.assert_array_equal(engine.oct_array("mult")[first:], t["mult"][first:])
    np.testing.assert_array_equal(pv, r["pv32"])
    tag = S.case_id(case)
    occupied = np.flatnonzero(t["mult"][first:] > 0) + first
    # centroids: fp32 sums in another order than the oracle's.  The oracle adds a cell's particles one after the other (thousands of
    # equal z on plane_off: 1e-5 of the coordinate is lost), so the yardstick is the fp64 oracle: no further from it than twice the
    # fp32 oracle is, plus 2e-7 of the largest coordinate (three roundings of an fp32 mean).
    c64 = r["t64"]["ex"]["center"]
    cscale = np.abs(c64[occupied]).max() + 1e-300
    cerr = np.abs(engine.oct_array("center4")[occupied, :3] - c64[occupied]).max() / cscale
    cfloor = np.abs(t["ex"]["center"][occupied] - c64[occupied]).max() / cscale
    print("%s: centres gpu-oracle64 %.3e oracle32-oracle64 %.3e of the largest coordinate" % (tag, cerr, cfloor))
    assert cerr < 2 * cfloor + 2e-7
    print("%s: L %d, %d occupied leaf cells" % (tag, info.L, len(np.unique(t["keys"]))))
    if what != "forces":
        print("%s (no assertion): gpu-oracle32 %.3e gpu-oracle64 %.3e floor %.3e" % (tag, force_err(a, r["a32"]), force_err(a, r["a64"]), r["floor"]))
        return
    got = {"mpole": engine.oct_array("mpole"), "local": engine.oct_array("local")}
    if overflow:
        e64 = force_err(a, r["a64"])
        print("%s far_fp64: gpu64-oracle64 %.3e" % (tag, e64))
        assert np.isfinite(a).all()
        assert e64 < 1e-5
        # Locals of the occupied cells against the fp64 oracle, 2e-5 as in test_far_fp64_against_double_oracle -- but not column by
        # column throughout: three particles on the axes and a ball at the origin make most components of an order vanish by
        # symmetry (1e-5 .. 1e-12 of the order's largest), and what is left in them is the rounding of the ball's fp32 centroid.
        # That rounding (6e-8 of a coordinate, seen k + 1 <= 11 times by an order-k coefficient: 7e-7 of the order's scale) is more
        # than 1.3e-5 of a column smaller than 1 / 20 of its order's largest.  So: every column relative to its ORDER's largest
        # entry, and the columns above 1 / 20 of that relative to their own.
        g, w = got["local"][occupied], r["t64"]["ex"]["local"][occupied]
        col = np.abs(w).max(axis=0)
        order = np.floor(np.sqrt(np.arange(w.shape[1]))).astype(int)          # order q holds columns q^2 .. (q + 1)^2 - 1
        oscale = np.array([col[order == q].max() for q in order]).clip(1e-300)
        by_order = (np.abs(g - w) / oscale).max()
        own = S.column_errs(g, w)[col >= 0.05 * oscale].max()
        print("%s far_fp64: local gpu64-oracle64 %.3e of the order's scale, %.3e of the column's (%d of %d columns)"
              % (tag, by_order, own, (col >= 0.05 * oscale).sum(), len(col)))
        assert by_order < 2e-5 and own < 2e-5
        return
    assert_forces(tag, a, r)
    for name in ("mpole", "local"):
        w32, w64 = r["t32"]["ex"][name][occupied], r["t64"]["ex"][name][occupied]          # (a column's scale: its largest entry over the occupied cells)
        alive = S.alive_columns(w32, w64)
        floor = S.column_errs(w32, w64)[alive].max()
        err = S.column_errs(got[name][occupied], w64)[alive].max()
        print("%s: %s gpu-oracle64 %.3e, oracle32-oracle64 %.3e (%d of %d columns)" % (tag, name, err, floor, alive.sum(), len(alive)))
        assert err < 2 * floor + 2e-5, name
