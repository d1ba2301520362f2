"""CPU tests: pin the oracle against the reference outputs recorded in BASELINE.md / SURVEY.md
(tests/golden/reference_recorded.json) and against closed-form invariants."""
import json
import os

import numpy as np
import pytest

from nbutil import canon_pairs, force_err, kd_admissible_f32, leaf_pair_cover, list_entries_changed

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLD, "reference_recorded.json")) as f:
        return json.load(f)


def test_reference_test_mode_error_table(oracle32, recorded):
    """`nbco3 -cpu -n 4096 -test`: the oracle reproduces all ten recorded mean relative errors."""
    o = oracle32
    rec = recorded["test_mode_relerr"]
    n = rec["n"]
    buf = o.init_reference(n, test_mode=True)
    par = o.params(n)
    ref = o.direct3(buf[0], par, threads=4)
    for p, want in enumerate(rec["values"], start=1):
        _, a = o.fmm_kd(buf[:2], par, p=p, threads=4, unsort=True)
        got = o.mean_relerr(a, ref)
        # recorded values carry 4 significant digits
        assert abs(got - want) <= 6e-4 * want, (p, got, want)


@pytest.mark.parametrize("n", [4096, 32768])
def test_reference_interaction_lists(oracle32, recorded, n):
    """List sizes and directed pair counts recorded from the reference's CPU traversal (exact)."""
    o = oracle32
    rec = recorded["gaussian_p6_lists"][str(n)]
    buf = o.init_reference(n)
    _, _ = o.fmm_kd(buf[:2], o.params(n), p=6, threads=4, unsort=False)
    t = o.kd_tree()
    assert t["L"] == rec["L"]
    assert len(t["p2p"]) == rec["p2p"]
    assert len(t["m2l"]) == rec["m2l"]
    mult = t["mult"].astype(np.int64)
    pairs = int((2 * mult[t["p2p"][:, 0]] * mult[t["p2p"][:, 1]]).sum() + (mult[(1 << t["L"]) - 1:] ** 2).sum())
    assert pairs == rec["pairs"]


def test_kd_ranges_and_mult(oracle32):
    """index[j] = ceil(n i / 2^l) (fmm_cart3_kdtree.cuh:117-118), mult = differences (appel.cuh:184-197)."""
    o = oracle32
    for n in (4096, 5000, 30001):
        buf = o.init_reference(n)
        o.fmm_kd(buf[:2], o.params(n), p=4, threads=2, unsort=True)
        t = o.kd_tree()
        L = t["L"]
        assert L == o.lib.oracle_kd_levels(n, 4, 1.0)
        for l in range(1, L + 1):
            m = 1 << l
            want = np.array([0 if i == 0 else (n * i - 1) // m + 1 for i in range(m)])
            np.testing.assert_array_equal(t["index"][m - 1:2 * m - 1], want)
        leaves = t["mult"][(1 << L) - 1:]
        assert leaves.sum() == n and leaves.max() - leaves.min() <= 1
        assert t["mult"][0] == n


def test_direct_variants_agree_with_fp64(oracle32, oracle64):
    o32, o64 = oracle32, oracle64
    n = 2048
    buf = o32.init_reference(n)
    par32 = o32.params(n)
    a3 = o32.direct3(buf[0], par32)
    a2 = o32.direct2(buf[0], par32, threads=3)
    a64 = o64.direct3(buf[0].astype(np.float64), o64.params(n))
    assert force_err(a3, a64) < 1e-6
    assert force_err(a2, a64) < 2e-5
    # the self term contributes exactly zero (direct.cuh:160, d = 0)
    one = o32.direct3(buf[0][:1], par32)
    assert np.all(one == 0)


def test_fmm_converges_to_direct(oracle32):
    o = oracle32
    n = 4096
    buf = o.init_reference(n)
    par = o.params(n)
    ref = o.direct3(buf[0], par, threads=4)
    errs = []
    for p in (2, 4, 6, 8, 10):
        _, a = o.fmm_kd(buf[:2], par, p=p, threads=1, unsort=True)
        errs.append(o.mean_relerr(a, ref))
    assert all(errs[i + 1] < errs[i] for i in range(len(errs) - 1)), errs
    assert errs[2] < 3e-3 and errs[-1] < 1e-4, errs     # 1.36e-3 (p=6), 2.8e-5 (p=10) on another ball


def test_fmm_thread_count_only_changes_rounding(oracle32):
    o = oracle32
    n = 4096
    buf = o.init_reference(n)
    par = o.params(n)
    _, a1 = o.fmm_kd(buf[:2], par, p=5, threads=1, unsort=True)
    _, a1b = o.fmm_kd(buf[:2], par, p=5, threads=1, unsort=True)
    _, a8 = o.fmm_kd(buf[:2], par, p=5, threads=8, unsort=True)
    np.testing.assert_array_equal(a1, a1b)              # single thread is bit-reproducible
    assert np.abs(a8 - a1).max() <= 2e-5 * np.abs(a1).max()


def test_unsort_false_permutes_velocities_consistently(oracle32):
    o = oracle32
    n = 1000
    buf = o.init_reference(n)
    par = o.params(n)
    pv, a = o.fmm_kd(buf[:2], par, p=3, threads=1, unsort=False)
    perm = o.kd_unsort(n)
    np.testing.assert_array_equal(pv[0], buf[0][perm])
    np.testing.assert_array_equal(pv[1], buf[1][perm])
    _, a_u = o.fmm_kd(buf[:2], par, p=3, threads=1, unsort=True)
    np.testing.assert_array_equal(a, a_u[perm])


def test_octree_traceless_accuracy(oracle32):
    """octree-traceless mean error 2.6e-4 (p=6) / 1.3e-5 (p=10) at N=4096."""
    o = oracle32
    n = 4096
    buf = o.init_reference(n)
    par = o.params(n)
    for p, bound in ((6, 8e-4), (10, 6e-5)):
        pv, a = o.fmm_oct_traceless(buf[:2], par, p=p, threads=4)
        ref = o.direct3(pv[0], par, threads=4)
        assert o.mean_relerr(a, ref) < bound


def test_integrators_order_and_energy(oracle64):
    """integrator.cuh:32-167: energy error of Euler / leapfrog / Forest-Ruth / PEFRL shrinks with
    the scheme's order when dt is halved (smooth potential: EPS2 = 1e-4)."""
    from oracle import pyoracle as po
    o = oracle64
    n, eps2 = 64, 1e-4
    base = o.init_reference(n)
    par = o.params(n)

    def drift(scheme, dt):
        buf = base.copy()
        o.compute_force(po.KIND_DIRECT3, buf, par, eps2=eps2)
        e0 = o.energy(buf, par, eps2=eps2).sum()
        for _ in range(int(round(2.0 / dt))):
            o.integrate(scheme, po.KIND_DIRECT3, buf, par, dt, eps2=eps2)
        return abs(o.energy(buf, par, eps2=eps2).sum() - e0) / abs(e0)

    for scheme, min_ratio in ((po.SCHEME_EULER, 1.5), (po.SCHEME_LEAPFROG, 3.2), (po.SCHEME_FR, 12.0), (po.SCHEME_PEFRL, 12.0)):
        e1, e2 = drift(scheme, 0.2), drift(scheme, 0.1)
        assert e1 / e2 > min_ratio, (scheme, e1, e2)
    # pre_symplectic_euler is F K D: one step equals compute_force + K + D
    a = base.copy(); b = base.copy()
    o.integrate(po.SCHEME_PRE_EULER, po.KIND_DIRECT3, a, par, 0.01, eps2=eps2)
    o.compute_force(po.KIND_DIRECT3, b, par, eps2=eps2)
    o.step(b[1], b[2], 0.01); o.step(b[0], b[1], 0.01)
    np.testing.assert_array_equal(a, b)


def test_init_reference_statistics(oracle32):
    """main3.cu:71-137: centred, RMS-normalised Gaussian ball."""
    o = oracle32
    n = 4096
    buf = o.init_reference(n)
    for arr, sig in ((buf[0], (0.003, 0.001, 0.01)), (buf[1], (0.003 * 1.095, 0.001, 0.01))):
        assert np.abs(arr.mean(axis=0)).max() < 1e-7
        np.testing.assert_allclose(np.sqrt((arr.astype(np.float64) ** 2).mean(axis=0)), sig, rtol=1e-4)


# ---- the GPU driver's two modes (fmm_cart3_kdtree.cuh:429-547 with b_m2l_first = true, :1619-1645 tree reuse) -------------------
# (n, p, uniform cube, dt of the reuse steps): the inputs the traversal pins below run on; L = 7, 9 and 10
DRIVER_INPUTS = [(4096, 6, False, 5e-3), (5000, 3, True, 0.1), (30001, 5, False, 2e-2)]


def oracle_schedule(o, buf, par, p, tree_steps, m2l_first, dt, evals, threads=4, **kw):
    """The oracle driving itself through leapfrog as the reference's GPU loop does (force, then per step: kick, drift, force,
    kick), rebuilding at every tree_steps-th evaluation and reusing the tree in between.  Yields (k, state, Coulomb part of the
    accelerations, tree dict) after every evaluation; the state [pos | vel | acc] is in tree order."""
    d = np.array(buf, dtype=o.dtype, copy=True)
    dt = float(np.float32(dt))
    offM, offL = p * (p + 1) * (p + 2) // 6, (p + 1) ** 2
    for k in range(evals):
        if k:
            o.step(d[1], d[2], dt / 2)
            o.step(d[0], d[1], dt)
        pv, a = o.fmm_kd(d[:2], par, p=p, unsort=False, m2l_first=m2l_first, reuse=int(k % tree_steps != 0), threads=threads, **kw)
        d[:2] = pv
        d[2] = a
        tree = o.kd_tree(offM=offM, offL=offL)
        tree["unsort"] = o.kd_unsort(d.shape[1])
        yield k, d, a, tree
        o.add_elastic(d[0], d[2], par[3:])
        if k:
            o.step(d[1], d[2], dt / 2)


@pytest.mark.parametrize("n,p,cube,dt", DRIVER_INPUTS)
@pytest.mark.parametrize("m2l_first", [0, 1])
def test_every_leaf_pair_is_served_exactly_once(oracle32, n, p, cube, dt, m2l_first):
    """Both traversal orders, on a fresh tree and on a reused one (new centres, stale boxes): the node pairs of the two lists,
    expanded to the leaf pairs below them, plus the self pairs tile the nleaf x nleaf matrix exactly once.  Independent of the
    opening criterion: it only sees whether the recursion loses or duplicates a branch."""
    o = oracle32
    buf = o.init_reference(n, test_mode=cube)
    assert o.lib.oracle_kd_levels(n, p, 1.0) <= 11
    for k, _, _, tree in oracle_schedule(o, buf, o.params(n), p, 3, m2l_first, dt, 3):
        cover = leaf_pair_cover(tree)
        assert cover.min() == 1 and cover.max() == 1, (k, int(cover.min()), int(cover.max()))


@pytest.mark.parametrize("n,p,cube,dt", DRIVER_INPUTS)
def test_m2l_first_moves_leaf_pairs_from_p2p_to_m2l(oracle32, recorded, n, p, cube, dt):
    """m2l_first = 1 asks the opening criterion before the leaf test, so the only thing that may change against the default
    order is that admissible LEAF pairs become M2L entries: its P2P list is a subset of the default one, the pairs that left it
    are exactly what its M2L list gained, and there are many of them (19 % - 57 % of the P2P list on these inputs).  Every M2L
    entry, fresh and under reuse, meets the opening criterion recomputed in float32 numpy, and no P2P entry of the M2L-first
    order does."""
    o = oracle32
    buf = o.init_reference(n, test_mode=cube)
    par = o.params(n)
    o.fmm_kd(buf[:2], par, p=p, threads=4, unsort=False, m2l_first=0)
    t0 = o.kd_tree()
    if (n, p) == (4096, 6):   # the reference's recorded list sizes are those of its CPU traversal
        rec = recorded["gaussian_p6_lists"]["4096"]
        assert (len(t0["p2p"]), len(t0["m2l"])) == (rec["p2p"], rec["m2l"])
    o.fmm_kd(buf[:2], par, p=p, threads=4, unsort=False, m2l_first=1)
    t1 = o.kd_tree()
    for name in ("index", "mult", "splitdim", "lbound", "rbound", "center"):
        np.testing.assert_array_equal(t1[name], t0[name], err_msg=name)
    p2p0, m2l0, p2p1, m2l1 = canon_pairs(t0["p2p"]), canon_pairs(t0["m2l"]), canon_pairs(t1["p2p"]), canon_pairs(t1["m2l"])
    assert np.isin(p2p1, p2p0).all()
    assert np.isin(m2l0, m2l1).all()
    moved = np.setdiff1d(p2p0, p2p1)
    np.testing.assert_array_equal(moved, np.setdiff1d(m2l1, m2l0))
    assert len(moved) >= 0.10 * len(p2p0), (len(moved), len(p2p0))
    leaf0 = (1 << t1["L"]) - 1
    assert ((moved >> 32) >= leaf0).all() and ((moved & 0xFFFFFFFF) >= leaf0).all()
    checked = 0
    for order in (0, 1):
        for k, _, _, tree in oracle_schedule(o, buf, par, p, 3, order, dt, 3):
            assert kd_admissible_f32(tree, tree["m2l"], p).all(), (order, k)
            if order == 1:
                assert not kd_admissible_f32(tree, tree["p2p"], p).any(), k
                both_leaves = (np.asarray(tree["m2l"]) >= leaf0).all(axis=1)
                checked += int(both_leaves.sum())
    assert checked > 1000, checked


def test_reuse_at_unmoved_positions_is_the_same_evaluation(oracle32):
    """A reuse evaluation skips the sorts and the boxes and nothing else: given the tree-ordered state of evaluation 0 again, it
    reproduces evaluation 0 bit for bit (single thread: no atomics), for both traversal orders."""
    o = oracle32
    n, p = 5000, 5
    buf = o.init_reference(n)
    par = o.params(n)
    offM, offL = p * (p + 1) * (p + 2) // 6, (p + 1) ** 2
    for m2l_first in (0, 1):
        pv0, a0 = o.fmm_kd(buf[:2], par, p=p, threads=1, unsort=False, m2l_first=m2l_first)
        t0, perm0 = o.kd_tree(offM=offM, offL=offL), o.kd_unsort(n)
        pv1, a1 = o.fmm_kd(pv0, par, p=p, threads=1, unsort=False, m2l_first=m2l_first, reuse=1)
        t1, perm1 = o.kd_tree(offM=offM, offL=offL), o.kd_unsort(n)
        np.testing.assert_array_equal(pv1, pv0)
        np.testing.assert_array_equal(a1, a0)
        np.testing.assert_array_equal(perm1, perm0)
        assert sorted(t1) == sorted(t0)
        for name in t0:
            np.testing.assert_array_equal(t1[name], t0[name], err_msg=name)


def test_reuse_keeps_the_topology_and_refuses_a_foreign_tree(oracle32):
    """After real steps a reuse evaluation still has the index / splitdim / boxes / permutation of the rebuild (stale boxes are
    the reference's behaviour: evalBox runs inside the rebuild block only, fmm_cart3_kdtree.cuh:1619-1642), new centres and new
    lists, positions and velocities as the caller gave them.  It is refused when there is no tree-ordered tree of the same n, p
    and depth to reuse, and a refusal leaves the stored tree alone."""
    o = oracle32
    n, p = 8192, 4
    buf = o.init_reference(n)
    par = o.params(n)
    first = None
    for k, d, _, tree in oracle_schedule(o, buf, par, p, 4, 1, 5e-3, 4):
        if k == 0:
            first = tree
            continue
        for name in ("index", "splitdim", "lbound", "rbound", "unsort", "mult"):
            np.testing.assert_array_equal(tree[name], first[name], err_msg=name)
        assert not np.array_equal(tree["center"], first["center"])
        assert list_entries_changed(first, tree) > 0
        inside = (d[0] >= tree["lbound"][0]).all() and (d[0] <= tree["rbound"][0]).all()
    assert not inside          # the ball has moved out of the root box it was built with, and the box has stayed
    state = d[:2].copy()
    # the caller's positions and velocities pass through a reuse evaluation untouched
    pv, _ = o.fmm_kd(state, par, p=p, unsort=False, m2l_first=1, reuse=1)
    np.testing.assert_array_equal(pv, state)
    before = o.kd_tree()
    for kw in (dict(p=p + 1), dict(p=p, unsort=True), dict(p=p, dens_inhom=4.0)):
        okw = dict(unsort=False, m2l_first=1, reuse=1)
        okw.update(kw)
        rc, _, _ = o.fmm_kd_rc(state, par, **okw)
        assert rc != 0, kw
    rc, _, _ = o.fmm_kd_rc(state[:, :n - 1], o.params(n - 1), p=p, unsort=False, reuse=1)
    assert rc != 0
    after = o.kd_tree()
    for name in before:
        np.testing.assert_array_equal(after[name], before[name], err_msg=name)
    # a tree built with unsort = 1 leaves the caller's order behind: nothing to reuse either
    o.fmm_kd(buf[:2], par, p=p, unsort=True)
    rc, _, _ = o.fmm_kd_rc(buf[:2], par, p=p, unsort=False, reuse=1)
    assert rc != 0


def test_reuse_keeps_the_physics(oracle32):
    """The `-test2` configuration (main3.cu:812-831; N = 8192, p = 4, the GPU traversal order, a rebuild every 8 evaluations,
    dt = 5e-4): across the reuse evaluations the mean error against the direct sum stays below 1.5 x that of the evaluation
    that built the tree, the margin tests/test_cli.py gives the binary."""
    o = oracle32
    n, p = 8192, 4
    buf = o.init_reference(n)
    par = o.params(n)
    errs = []
    for k, d, a, _ in oracle_schedule(o, buf, par, p, 8, 1, 5e-4, 8):
        errs.append(o.mean_relerr(a, o.direct3(d[0], par, threads=4)))
    assert 0 < errs[0] < 0.1
    assert max(errs) < 1.5 * errs[0], errs
