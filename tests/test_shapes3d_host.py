"""CPU tests: what the two oracles do on the inputs of shapes3d.CASES, asserted before any GPU is involved.

test_gpu_shapes3d.py compares GPU evaluations of these inputs with the oracles under bounds taken from the oracles.  That is only a
test where the oracles themselves are sound on the input, where the shape really is degenerate in the way its name says, and where
the bound is tight enough to tell a wrong evaluation from a right one.  Every one of these is asserted here, per case.

The last part does the same for shapes3d.SELECT_CASES and test_gpu_select_shapes.py: class and floor of every row, the ties and the
bucket fill at every node that the GPU builds by selection, the build_mode that follows, and the order of cut ties."""
import numpy as np
import pytest

import shapes3d as S
from nbutil import expansion_err, force_err, leaf_pair_cover

FORCES = [c for c in S.CASES if c[4] == "forces"]
LISTS = [c for c in S.CASES if c[4] == "lists"]


def test_the_table_covers_what_it_has_to():
    """at least 12 kd-tree and 10 octree "forces" cases; every shape on which forces mean something in at least one of them per
    evaluator family; every "lists" case with a stated reason; no case twice"""
    assert len(set(S.CASES)) == len(S.CASES)
    kd = [c for c in FORCES if c[0] == "kd"]
    oc = [c for c in FORCES if c[0] != "kd"]
    assert len(kd) >= 12 and len(oc) >= 10
    # (the shapes added with SELECT_CASES run there only: test_the_select_table_covers_what_it_has_to)
    need = set(S.SHAPES) - set(S.SELECT_ONLY) - {"two_clumps", "offset", "dup64"}
    assert len(need) == 10
    assert need <= {c[1] for c in kd}
    assert need <= {c[1] for c in oc}
    assert {c[:4] for c in LISTS} == set(S.LISTS_WHY)
    assert S.OCT_FP32_OVERFLOWS <= {c[:4] for c in oc}
    assert S.FLOOR_CASE_OF_LONG_RANGE in {c[:4] for c in kd}


def test_states_are_deterministic_and_keep_the_ball(oracle32):
    """a shape does not depend on what was built before it; velocities and the particle count are the Gaussian ball's; float32"""
    n = 4096
    base = oracle32.init_reference(n)
    first = {name: S.state(oracle32, name, n) for name in S.SHAPES}
    for name in reversed(S.SHAPES):
        b = S.state(oracle32, name, n)
        np.testing.assert_array_equal(b, first[name])
        np.testing.assert_array_equal(b[1], base[1])
        assert b.shape == (3, n, 3) and b.dtype == np.float32 and not b[2].any()
    np.testing.assert_array_equal(first["gauss"], base)
    assert len(np.unique(first["dup8"][0], axis=0)) == n // 8 and len(np.unique(first["lattice"][0], axis=0)) == n
    assert len(np.unique(first["quant16"][0])) <= 33


@pytest.mark.parametrize("case", FORCES, ids=S.case_id)
def test_a_forces_case_has_sound_oracles(oracle32, oracle64, case):
    """kd-tree: both oracles finite, same tree integers, same permutation, same P2P / M2L lists in fp32 and fp64, every ordered leaf
    pair served exactly once.  Octree: the fp64 oracle finite, the fp32 oracle finite except on the cases named in
    OCT_FP32_OVERFLOWS, same sorted keys and permutation."""
    r = S.evaluate(oracle32, oracle64, case)
    print("%s floor %.3e" % (S.case_id(case), r["floor"]))
    assert r["finite64"]
    if case[0] == "kd":
        assert r["finite32"]
        assert S.same_kd_tree(r["t32"], r["t64"])
        assert S.same_kd_lists(r["t32"], r["t64"])
        cover = leaf_pair_cover(r["t32"])
        assert cover.min() == 1 and cover.max() == 1
        # the floors the bounds are built on stay at rounding level: nothing here widens the project's bar by more than 1.5
        assert r["floor"] < 3.75e-6
    else:
        assert r["finite32"] == (case[:4] not in S.OCT_FP32_OVERFLOWS)
        np.testing.assert_array_equal(r["t32"]["keys"], r["t64"]["keys"])
        np.testing.assert_array_equal(r["t32"]["perm"], r["t64"]["perm"])
        np.testing.assert_array_equal(r["pv32"], r["pv64"].astype(np.float32))
        if r["finite32"]:
            assert r["floor"] < 1.25e-5
    # multipole / local columns on which fp32 says nothing (shapes3d.alive_columns): only where a moment vanishes by symmetry, and
    # then by a wide margin -- the oracles agree to 1e-3 on every other column and differ by more than 100 % on these
    if r["finite32"]:
        for name in ("mpole", "local"):
            if case[0] == "kd":
                w32, w64 = r["t32"][name], r["t64"][name]
            else:
                occ = np.flatnonzero(r["t32"]["mult"][9:] > 0) + 9
                w32, w64 = r["t32"]["ex"][name][occ], r["t64"]["ex"][name][occ]
            errs, alive = S.column_errs(w32, w64), S.alive_columns(w32, w64)
            print("%s %s: %d of %d columns alive, floor %.3e" % (S.case_id(case), name, alive.sum(), len(alive), errs[alive].max()))
            assert errs[alive].max() < 1e-3 and (errs[~alive] > 1).all()
            assert alive.all() or case[1] in ("plane_off", "lattice")
            assert 4 * alive.sum() >= len(alive) and alive[0]


@pytest.mark.parametrize("case", LISTS, ids=S.case_id)
def test_a_lists_case_is_one_for_its_stated_reason(oracle32, oracle64, case):
    """the inputs on which a force comparison says nothing about a kernel, each with the measurement that excludes it; the lists of
    the fp32 oracle are still a complete cover (kd-tree), the keys still agree (octree)"""
    r = S.evaluate(oracle32, oracle64, case)
    why = S.LISTS_WHY[case[:4]]
    print("%s %s floor %.3e" % (S.case_id(case), why, r["floor"]))
    if case[0] == "kd":
        cover = leaf_pair_cover(r["t32"])
        assert cover.min() == 1 and cover.max() == 1
        same = S.same_kd_tree(r["t32"], r["t64"]) and S.same_kd_lists(r["t32"], r["t64"])
    else:
        np.testing.assert_array_equal(r["t32"]["keys"], r["t64"]["keys"])
        same = True
    if why == "nonfinite32":
        assert not r["finite32"] and r["finite64"] and same
    elif why == "nonfinite":
        assert not r["finite32"] and not r["finite64"] and same
    elif why == "lists_differ":
        assert r["finite32"] and r["finite64"] and not same
        assert r["floor"] > 5e-5          # and the forces show it
    else:
        assert why == "cancellation" and same and r["floor"] > 5e-5


def wrong_references(o, case, r):
    """accelerations of three evaluations that are NOT the case's: one order less, no near field, a wider opening radius"""
    ev, p = case[0], r["p"]
    kws = [("order p - 1", p - 1, {}), ("coll = False", p, dict(coll=False))]
    if case[3] < 10:
        kws.append(("radius 2", p, dict(radius=2.0)))
    return [(name, S.run_oracle(o, ev, r["buf"], r["par"], pp, expansions=False, **kw)[0]) for name, pp, kw in kws]


@pytest.mark.parametrize("case", FORCES, ids=S.case_id)
def test_the_bound_tells_a_wrong_evaluation_from_a_right_one(oracle32, oracle64, case):
    """Each deliberately wrong reference is at least 10 x the case's bound away from the right one -- fp32 references against
    max(1e-5, 4 floor); on the octree cases where fp32 overflows, fp64 references against the 1e-5 of the far_fp64 comparison.

    Octree, OCT_NEAR_FIELD_ONLY shapes: the far field is too small a part of the force for ANY force bound to see it (order p - 1
    and radius 2 move the accelerations by less than the bound; asserted, so that nobody reads those force checks as far-field
    checks).  What the far field does there is compared through the locals: a radius-2 evaluation moves the locals of the occupied
    cells by more than 10 x the bound the GPU module puts on them."""
    r = S.evaluate(oracle32, oracle64, case)
    o, a = (oracle32, r["a32"]) if r["finite32"] else (oracle64, r["a64"])
    bound = S.force_bound(r["floor"]) if r["finite32"] else 1e-5
    near_only = case[0] != "kd" and case[1] in S.OCT_NEAR_FIELD_ONLY
    for name, aw in wrong_references(o, case, r):
        err = force_err(aw, a)
        print("%s %s: %.3e = %.1f x bound" % (S.case_id(case), name, err, err / bound))
        if near_only and name != "coll = False":
            assert err < bound, name
        else:
            assert not err <= 10 * bound, name          # (a NaN reference -- dup16 at order 3, whose 8-particle leaves coincide -- fails every bound)
    if near_only:
        tag = "32" if r["finite32"] else "64"
        t = r["t" + tag]
        occ = np.flatnonzero(t["mult"][9:] > 0) + 9
        _, _, t2 = S.run_oracle(o, case[0], r["buf"], r["par"], r["p"], radius=2.0)
        np.testing.assert_array_equal(t2["keys"], t["keys"])
        moved = expansion_err(t2["ex"]["local"][occ], t["ex"]["local"][occ])
        lbound = 2e-5 if not r["finite32"] else 2 * expansion_err(r["t32"]["ex"]["local"][occ].astype(np.float64), r["t64"]["ex"]["local"][occ]) + 2e-5
        print("%s locals moved by radius 2: %.3e, bound %.3e" % (S.case_id(case), moved, lbound))
        if case[1] == "two_clumps":
            assert moved == 0          # two occupied cells 1000 R apart: one M2L at the top, whatever the radius
        else:
            assert moved > 10 * lbound


# ---- the shape is what its name says ---------------------------------------------------------------------------------------------
def kd_case(shape, n, p):
    (c,) = [c for c in S.CASES if c[:4] == ("kd", shape, n, p)]
    return c


@pytest.mark.parametrize("shape,n,p", [("plane", 4096, 4), ("plane", 8000, 6), ("plane", 4096, 10), ("plane_off", 4096, 4), ("plane_off", 8000, 6)])
def test_plane_every_box_has_zero_thickness(oracle32, oracle64, shape, n, p):
    t = S.evaluate(oracle32, oracle64, kd_case(shape, n, p))["t32"]
    np.testing.assert_array_equal(t["lbound"][:, 2], t["rbound"][:, 2])
    assert (t["splitdim"] != 2).all()
    assert ((t["rbound"] - t["lbound"])[:, :2] > 0).any()


@pytest.mark.parametrize("n,p", [(4096, 4), (8000, 6)])
def test_line_every_box_is_a_segment(oracle32, oracle64, n, p):
    t = S.evaluate(oracle32, oracle64, kd_case("line", n, p))["t32"]
    np.testing.assert_array_equal(t["lbound"][:, 1:], t["rbound"][:, 1:])
    assert (t["splitdim"] == 0).all()


@pytest.mark.parametrize("n,p", [(4096, 4), (2197, 4), (8000, 6)])
def test_lattice_ties_at_the_root_median(oracle32, oracle64, n, p):
    """a whole lattice plane of m^2 particles shares the root's median coordinate: the cut goes through exact ties"""
    r = S.evaluate(oracle32, oracle64, kd_case("lattice", n, p))
    m = S.lattice_side(n)
    x = r["buf"][0][:, int(r["t32"]["splitdim"][0])]
    median = np.sort(x)[n // 2]
    assert (x == median).sum() >= m * m
    # an odd side puts the cut itself inside the tied plane; an even one between two planes (16 = 2^4: every cut of the tree does)
    assert (np.sort(x)[n // 2 - 1] == median) == (m % 2 == 1)


def points_per_node(r, level):
    """distinct positions in every node of a level, from the state in the fp32 oracle's tree order"""
    t = r["t32"]
    pos = r["buf"][0][t["perm"]]
    beg = (1 << level) - 1
    return np.array([len(np.unique(pos[i:i + m], axis=0)) for i, m in zip(t["index"][beg:2 * beg + 1], t["mult"][beg:2 * beg + 1])])


@pytest.mark.parametrize("shape,n,p,k", [("dup2", 4096, 4, 2), ("dup8", 4096, 4, 8), ("dup8", 8000, 6, 8), ("dup16", 4096, 4, 16), ("dup64", 4096, 4, 64)])
def test_duplicates_share_leaves(oracle32, oracle64, shape, n, p, k):
    """K copies of n / K points.  The boxes of this tree are cut boxes (a child inherits its parent's box and is cut along one axis,
    fmm_cart3_kdtree.cuh:109-137), not bounding boxes, so coincident particles do NOT give lbound == rbound: no leaf of dup2 / dup8 /
    dup16 has a zero-size box, and one leaf of dup64 has.  What duplication does give: leaves of a few distinct points (one point
    from 16 copies on: leaf centroid = every particle, zero multipoles above order 0), copies of one point on both sides of a cut
    where n / K does not divide into the leaves (8000: the median falls between exactly equal keys), and from 32 copies on
    neighbouring leaves with the same centroid (dist2 == 0 in the opening criterion)."""
    r = S.evaluate(oracle32, oracle64, kd_case(shape, n, p))
    t = r["t32"]
    L = t["L"]
    beg = (1 << L) - 1
    pts = points_per_node(r, L)
    mult = t["mult"][beg:]
    zero_box = int((t["lbound"][beg:] == t["rbound"][beg:]).all(axis=1).sum())
    print("%s n=%d: %d..%d distinct points in leaves of %d..%d, %d zero-size leaf boxes" % (shape, n, pts.min(), pts.max(), mult.min(), mult.max(), zero_box))
    assert (pts <= mult // k + 6).all()          # whole groups of copies, and at most one cut group per face of the leaf's box
    assert zero_box == (1 if shape == "dup64" else 0)
    if n % (k << L) == 0 or k >= mult.max():
        assert (pts == np.maximum(mult // k, 1)).all()          # the cuts fall between groups of copies
    else:
        assert pts.sum() > n // k                                 # some point has copies in two leaves: a cut through exact ties
    if k >= 16:
        c = t["center"][beg:]
        assert (pts == 1).all()
        assert ((c[0::2] == c[1::2]).all(axis=1)).all() == (k >= 32)          # sibling leaves on one point


@pytest.mark.parametrize("n,p", [(4096, 4), (8000, 6)])
def test_late_has_a_few_very_long_lists(oracle32, oracle64, n, p):
    """Three far particles: their leaves are partners of EVERY leaf, so the longest per-target list is the whole leaf level (256),
    three times the longest list of the ball itself.  With 256 leaves that cannot be 5 x the median (the stretched leaves also
    lengthen everybody else's list: median 92 / 103 against the ball's 28 / 38); the 5 x is asserted at the long-range size below,
    where the tree has 4096 leaves."""
    t = S.evaluate(oracle32, oracle64, kd_case("late", n, p))["t32"]
    ball = S.evaluate(oracle32, oracle64, kd_case("gauss", n, p))["t32"]
    per_target, control = S.per_target_entries(t), S.per_target_entries(ball)
    print("late n=%d p=%d: longest per-target list %d, median %d; ball: %d, %d" % (n, p, per_target.max(), np.median(per_target),
                                                                                control.max(), np.median(control)))
    assert per_target.max() == 1 << t["L"] == 256
    assert per_target.max() >= 2 * np.median(per_target) and per_target.max() >= 3 * control.max()


def test_late_at_the_long_range_size(oracle32):
    """the state of test_long_ranges_take_their_own_kernel_when_the_lists_are_long, with that test's three assertions on the
    oracle's lists: ranges far above 512 entries, a mean above the 48 that switches the long-range kernel on, 11..16 levels"""
    buf, par, pv, a, t = S.long_range_oracle(oracle32)
    n = S.LONG_RANGE["n"]
    ref = oracle32.init_reference(n)
    ref[0, :3] = S.LATE_ROWS * np.abs(ref[0]).max()
    np.testing.assert_array_equal(buf, ref)          # the construction of the existing test, bit for bit
    per_target = S.per_target_entries(t)
    assert per_target.max() > 2000 and per_target.mean() > 48 and 11 <= t["L"] + 1 <= 16, (per_target.max(), per_target.mean(), t["L"])
    print("late n=%d: %d leaf pairs, longest per-target list %d, median %d" % (n, len(t["p2p"]), per_target.max(), np.median(per_target)))
    assert per_target.max() >= 5 * np.median(per_target)
    assert np.isfinite(a).all()
    # the state it leaves (tree order) is a fixed point of the build: a context that rebuilds every step is given the same state from
    # its second evaluation on
    again = S.long_range_oracle(oracle32, again=True)
    np.testing.assert_array_equal(again[0][:2], pv)
    np.testing.assert_array_equal(again[2], pv)
    np.testing.assert_array_equal(again[4]["perm"], np.arange(n))
    assert S.same_kd_lists(again[4], t)
    cover = leaf_pair_cover(t)
    assert cover.min() == 1 and cover.max() == 1


# ---- what the reference does on 64 coincident copies -----------------------------------------------------------------------------
def test_dup64_lists_are_sound_and_the_forces_are_not(oracle32, oracle64):
    """dup64 at (4096, 4): 64 distinct points, 64 copies each.  In BOTH oracles the tree and the lists are finite and complete (cover
    1) and every acceleration is NaN -- so the GPU case compares trees and lists and says nothing about forces.

    Where the NaN comes from: not from the opening criterion.  Every M2L pair is well separated (the closest has dist2 = 2.3e-6, its
    larger box 1.8e-6); a pair of coincident nodes has dist2 = 0, which `parm^2 sz < dist2` never admits, so it is split down to a
    softened P2P.  The first non-finite locals are those of level 7 (nodes 127 .. 254), all of them, and they come from L2L: a
    level-6 node (63 .. 126) holds the 64 copies of ONE point, so both its children have exactly its centre, and the shift normalises
    d = centre[child] - centre[parent] = 0 by r = |d| = 0 (fmm_cart3_kdtree.cuh:1171-1194: d / r = NaN).  Nodes 63 -> 127 are the
    first such pair.  The same happens from 32 copies on (then the two 16-particle leaves of a level-7 node coincide) and not at 16
    copies, where a parent holds two different points; the fp64 oracle does the same arithmetic and fails the same way."""
    case = kd_case("dup64", 4096, 4)
    r = S.evaluate(oracle32, oracle64, case)
    for tag in ("32", "64"):
        t, a = r["t" + tag], r["a" + tag]
        L = t["L"]
        assert L == 8
        assert np.isnan(a).all()
        cover = leaf_pair_cover(t)
        assert cover.min() == 1 and cover.max() == 1
        assert np.isfinite(t["center"]).all() and np.isfinite(t["mpole"]).all()
        loc_ok = np.isfinite(t["local"]).all(axis=1)
        assert loc_ok[:127].all() and not loc_ok[127:].any()          # levels 0..6 finite, 7 and 8 not
        # level 6: one point per node (its cut box is not a point), both children exactly on the parent's centre
        lev6 = np.arange(63, 127)
        assert (points_per_node(r, 6) == 1).all()
        assert ((t["rbound"] - t["lbound"])[lev6].max(axis=1) > 0).all()
        np.testing.assert_array_equal(t["center"][2 * lev6 + 1], t["center"][lev6])
        np.testing.assert_array_equal(t["center"][2 * lev6 + 2], t["center"][lev6])
        assert (points_per_node(r, 5) == 2).all()          # ... and level 5 holds two points: its children's centres differ
        # no M2L pair is closer than its boxes are large: the far-field list itself is healthy
        m2l = t["m2l"].astype(np.int64).reshape(-1, 2)
        d2 = ((t["center"][m2l[:, 0]] - t["center"][m2l[:, 1]]) ** 2).sum(axis=1)
        sz = (t["rbound"] - t["lbound"]) ** 2
        sz = np.maximum(sz[m2l[:, 0]].sum(axis=1), sz[m2l[:, 1]].sum(axis=1))
        assert d2.min() > 1e-6 and (d2 > 0.25 * sz).all()


# ---- SELECT_CASES: the shapes at sizes whose top levels are built by selection ---------------------------------------------------
# (max ties, max bucket) over the selection nodes of the fp32 oracle's tree, as select_nodes counts them; "lists" rows too.  quant16:
# rounding to the grid leaves -0.0 and +0.0 behind, two keys of one coordinate -- 1127 + 1151 particles in the root pivot's bucket.
SELECT_TIES = {
    ("gauss", 20480, 4): (1, 1), ("plane", 20480, 4): (1, 1), ("plane_off", 20480, 4): (1, 1), ("line", 20480, 4): (1, 1),
    ("dup2", 20480, 4): (2, 2), ("dup8", 20480, 4): (8, 8), ("dup16", 20480, 4): (16, 16), ("late", 20480, 4): (1, 6),
    ("ejected", 20480, 4): (1, 12418), ("zeros", 20480, 4): (4, 8), ("lattice", 19683, 4): (729, 729), ("quant16", 20480, 4): (1979, 2278),
    ("dup64", 20480, 4): (64, 64), ("dup128", 20480, 4): (128, 128), ("two_clumps", 20480, 4): (1, 1), ("offset", 20480, 4): (3, 3),
    ("late", 20480, 6): (1, 6), ("dup8", 20480, 6): (8, 8), ("quant2048", 20480, 4): (18, 24),
    ("late", 65536, 4): (1, 10), ("plane", 65536, 4): (1, 2), ("line", 65536, 4): (1, 1), ("ejected", 65536, 4): (1, 39348),
}
# build_mode of a first build (shapes3d.mode_from_nodes); None: the figures leave it open
SELECT_MODES = {row[:3]: {0} for row in S.SELECT_CASES}
SELECT_MODES.update({("ejected", 20480, 4): {1}, ("ejected", 65536, 4): {1}, ("dup128", 20480, 4): {1}, ("lattice", 19683, 4): {2},
                     ("quant16", 20480, 4): {2}})


def test_the_select_table_covers_what_it_has_to():
    """every row has selection levels (three at about 20000 particles, four at 65536) and none of them is in CASES; every shape of
    the module at p = 4; late and dup8 also at p = 6; late, plane, line at 65536; every "lists" row with a stated reason"""
    rows = S.SELECT_CASES
    assert len(set(rows)) == len(rows)
    assert all(n > 2 * S.SELECT_MIN for _, n, _, _ in rows) and not {("kd",) + r for r in rows} & set(S.CASES)
    assert {s for s, n, p, _ in rows if p == 4 and n in (20480, 19683)} == set(S.SHAPES)
    assert all(n == (19683 if s == "lattice" else 20480) or n == 65536 for s, n, _, _ in rows) and 20480 % 128 == 0
    assert {("late", 20480, 6), ("dup8", 20480, 6), ("late", 65536, 4), ("plane", 65536, 4), ("line", 65536, 4)} <= {r[:3] for r in rows}
    assert {r[:3] for r in rows if r[3] == "lists"} == set(S.SELECT_LISTS_WHY)
    assert set(S.SELECT_LISTS_WHY.values()) <= {"nonfinite32", "nonfinite", "lists_differ", "cancellation"}
    assert set(SELECT_TIES) == set(SELECT_MODES) == {r[:3] for r in rows}
    assert set(S.SELECT_ONLY) <= {r[0] for r in rows} and not set(S.SELECT_ONLY) & {c[1] for c in S.CASES}


@pytest.mark.parametrize("row", S.SELECT_CASES, ids=S.select_id)
def test_a_select_case_is_what_the_table_says(oracle32, oracle64, row):
    """"forces": both oracles finite, same tree, permutation and lists, every ordered leaf pair served once, the floor at rounding
    level (plane_off: 1.35e-5, the cancellation of a plane at z = 0.37 R).  "lists": for the reason SELECT_LISTS_WHY states.  Every
    row: one selection level per halving above 4096 particles; the tie structure that the GPU module's build_mode expectation is
    built on, pinned as measured (SELECT_TIES), and the expectation itself (SELECT_MODES)."""
    shape, n, p, what = row
    r = S.evaluate(oracle32, oracle64, S.kd_of(row))
    t = r["t32"]
    same = S.same_kd_tree(t, r["t64"]) and S.same_kd_lists(t, r["t64"])
    cover = leaf_pair_cover(t)
    assert cover.min() == 1 and cover.max() == 1
    if what == "forces":
        assert r["finite32"] and r["finite64"] and same
        assert r["floor"] < (2e-5 if shape == "plane_off" else 3.75e-6)
    else:
        why = S.SELECT_LISTS_WHY[row[:3]]
        if why == "nonfinite":
            assert not r["finite32"] and not r["finite64"]
            assert S.same_kd_tree(t, r["t64"])
        else:
            assert why == "lists_differ" and r["finite32"] and r["finite64"] and not same
            assert r["floor"] > 5e-5
    nodes = S.select_nodes(t, r["buf"][0][t["perm"]])
    mode = S.expected_mode(oracle32, oracle64, row)
    print("%s floor %.3e, expected build_mode %s; selection nodes (node, ties, bucket, ties in the left child, bucket +- 1, warm bucket):\n%s"
          % (S.select_id(row), r["floor"], mode, nodes))
    levels = 3 if n < 65536 else 4
    np.testing.assert_array_equal(nodes[:, 0], np.arange((1 << levels) - 1))
    assert (nodes[:, 1] <= nodes[:, 2]).all() and (nodes[:, 2] <= nodes[:, 4]).all() and (nodes[:, 2] <= nodes[:, 5]).all()
    assert (1 <= nodes[:, 3]).all() and (nodes[:, 3] <= nodes[:, 1]).all()
    assert (int(nodes[:, 1].max()), int(nodes[:, 2].max())) == SELECT_TIES[row[:3]]
    assert mode == SELECT_MODES[row[:3]]
    if shape in ("dup64", "dup128"):
        # the two sides of kTieCap: 64 / 128 copies at EVERY selection node, alone in the pivot's bucket and its neighbours, and
        # every cut behind the tied run (20480 / 2^l is a multiple of 128)
        k = int(shape[3:])
        assert (nodes[:, 1:] == k).all()
    if shape == "ejected":
        assert nodes[0, 2] == (12418 if n == 20480 else 39348)          # the ball is a few buckets of the root's box
    if shape in ("dup2", "dup8", "dup16"):
        assert (nodes[:, 1] == int(shape[3:])).all() and (nodes[:, 3] == nodes[:, 1]).all()
    if shape == "lattice":
        assert (nodes[:, 3] < nodes[:, 1]).all()          # every cut inside a tied plane


@pytest.mark.parametrize("row", S.SELECT_CASES, ids=S.select_id)
def test_cut_ties_follow_the_sort_chain(oracle32, oracle64, row):
    """Wherever a cut of a selection node falls inside a run of equal keys, the tied particles of the oracle's left child are the
    first ones by (c[a2], c[a3], original index) -- the order the GPU's exact resolver is written to.  quant2048 is the row on which
    the SECOND key decides while the resolver is in charge (a dozen ties per node, build_mode 0): at two of its nodes the order
    without c[a2] picks other particles.  The other rows with cut ties either tie in all keys but the index (offset) or end in the
    sorting build (lattice, quant16)."""
    r = S.evaluate(oracle32, oracle64, S.kd_of(row))
    rows = S.tie_orders(r["t32"], r["buf"][0][r["t32"]["perm"]])
    print(S.select_id(row), rows)
    assert all(chain for _, chain, _ in rows)
    assert bool(rows) == (row[0] in ("lattice", "quant16", "offset", "quant2048"))
    if row[0] == "quant2048":
        assert [v for v, _, blind in rows if not blind] == [4, 5]
        assert S.expected_mode(oracle32, oracle64, row) == {0}


def test_zeros_puts_the_root_cut_between_the_two_zeros(oracle32, oracle64):
    """the root pivot is -0.0 and the right child begins at +0.0: the bounds of the root's children on the split axis are the two
    zeros, told apart by their bits only; four particles on each, all eight in one bucket of the linear key"""
    r = S.evaluate(oracle32, oracle64, S.kd_of(("zeros", 20480, 4, "forces")))
    t = r["t32"]
    a = int(t["splitdim"][0])
    ext = r["buf"][0].max(axis=0) - r["buf"][0].min(axis=0)
    assert a == int(np.argmax(ext))
    assert t["rbound"][1].view(np.uint32)[a] == 0x80000000
    assert t["lbound"][2].view(np.uint32)[a] == 0
    x = r["buf"][0][:, a]
    bits = x.view(np.uint32)
    assert (bits == 0x80000000).sum() == S.ZERO_BLOCK and (bits == 0).sum() == S.ZERO_BLOCK
    assert (x < 0).sum() == 20480 // 2 - S.ZERO_BLOCK and (x > 0).sum() == 20480 // 2 - S.ZERO_BLOCK
    np.testing.assert_array_equal(S.select_nodes(t, r["buf"][0][t["perm"]])[0, 1:5], [S.ZERO_BLOCK, 2 * S.ZERO_BLOCK, S.ZERO_BLOCK, 2 * S.ZERO_BLOCK])
    np.testing.assert_array_equal(r["buf"][1], oracle32.init_reference(20480)[1])


def test_the_bucket_restatement_against_exact_arithmetic():
    """lin_bucket rounds where k_kdselect.hip's lin_key rounds: against the same expression in exact rational arithmetic it is never
    more than one bucket off, is monotone, and sends the box faces to the first and the last bucket"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    lo, hi = np.float32(-0.731), np.float32(1.9)
    x = np.sort(rng.uniform(lo, hi, 2000).astype(np.float32))
    b = S.lin_bucket(x, lo, hi).astype(np.int64)
    assert (np.diff(b) >= 0).all()
    exact = np.array([int((Fraction(float(v)) - Fraction(float(lo))) / (Fraction(float(hi)) - Fraction(float(lo))) * 4294967040) >> 10 for v in x])
    assert np.abs(b - exact).max() <= 1
    assert S.lin_bucket(np.array([lo, hi]), lo, hi).tolist() == [0, 4294967040 >> 10]
    assert S.lin_bucket(np.array([lo, hi]), lo, lo).tolist() == [0, 0]          # a box of zero extent: one bucket
    np.testing.assert_array_equal(S.ordered_key(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32)),
                                  np.array([0x407FFFFF, 0x7FFFFFFF, 0x80000000, 0xBF800000], dtype=np.uint32))
