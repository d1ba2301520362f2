"""The selection build of the kd-tree (k_kdselect.hip: every level whose nodes hold more than 4096 particles) on the inputs of
shapes3d.SELECT_CASES -- flat, collinear, tied, duplicated, signed-zero, stretched and late-run states at 20480 and 65536 particles,
where the shapes of shapes3d.CASES (n <= 8000) only ever reach the LDS subtree build.  test_shapes3d_host.py shows, without a GPU,
what every row is: its class, its floor, the ties and the bucket fill at every selection node, and the build_mode that follows.

Bar: the fp32 oracle's tree, bit for bit -- integers, boxes and centres as bit patterns (-0.0 is not +0.0), permutation, both lists
as sets, the directed pair count -- whatever way the build took: two passes, three passes, the sorting build, or the warm one-pass
select around the previous build's pivots.  Every measured figure is printed (run with -s)."""
import numpy as np
import pytest

import shapes3d as S
from nbutil import assert_same_tree, canon_pairs, force_err, warm_engine
from test_gpu_shapes3d import assert_forces, dev, run_kd

pytestmark = pytest.mark.gpu

ROWS = {r[:3]: r for r in S.SELECT_CASES}
FUSED = [ROWS[(s, 20480, 4)] for s in ("plane", "line", "dup16", "late")]
TIED = [ROWS[("dup8", 20480, 4)], ROWS[("dup16", 20480, 4)]]
_warm = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def tree_bits(engine):
    """everything a build leaves behind, as integers"""
    t = {k: engine.kd_array(k).copy() for k in ("index", "mult", "splitdim", "unsort")}
    t.update({k: bits(engine.kd_array(k)) for k in ("lbound", "rbound", "center")})
    t.update({k: canon_pairs(engine.kd_array(k)) for k in ("p2p", "m2l")})
    info = engine.kd_info()
    t["counts"] = np.array([info.L, info.ntot, info.n, info.p2p_pairs, info.m2l_pairs, info.directed_p2p])
    return t


def assert_oracle_tree(engine, t, n, tag):
    """nbutil.assert_same_tree, and the boxes and centres once more as bit patterns: assert_array_equal calls -0.0 and 0.0 equal"""
    assert_same_tree(engine, t, n, t["perm"])
    for name in ("lbound", "rbound", "center"):
        np.testing.assert_array_equal(bits(engine.kd_array(name)), bits(t[name]), err_msg="%s %s (bits)" % (tag, name))


def assert_same_bits(t0, t1, tag):
    assert set(t0) == set(t1)
    for k in t0:
        np.testing.assert_array_equal(t0[k], t1[k], err_msg="%s %s" % (tag, k))


# ---- A. a fresh build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.SELECT_CASES, ids=S.select_id)
def test_fresh_select_build_is_the_oracles_tree(oracle32, oracle64, row):
    """unsort = 1 on a fresh context: the first build is cold, escalates as far as the input's ties send it (build_mode as
    shapes3d.expected_mode derives it from the oracle's tree) and ends on the oracle's tree; "forces" rows within the two bounds of
    test_gpu_shapes3d.  A second evaluation of the same input on the same context -- a warm build where the first stayed at two
    passes -- gives the same tree and the same accelerations bit for bit, and never a lower mode: escalation is sticky."""
    from coulomb_oscillators_amd import Engine
    shape, n, p, what = row
    tag = S.select_id(row)
    r = S.evaluate(oracle32, oracle64, S.kd_of(row))
    want_mode = S.expected_mode(oracle32, oracle64, row)
    eng = Engine()
    try:
        pv, a = run_kd(eng, r["buf"], r["par"], n, fmm_order=p, unsort=1)
        info = eng.kd_info()
        print("%s: build_mode %d (expected %s), %d leaf pairs, %d M2L pairs, warm builds %d misses %d"
              % (tag, info.build_mode, want_mode, info.p2p_pairs, info.m2l_pairs, info.warm_builds, info.warm_misses))
        assert_oracle_tree(eng, r["t32"], n, tag)
        np.testing.assert_array_equal(bits(pv), bits(r["buf"][:2]))
        if what == "forces":
            assert_forces(tag, a, r)
        elif r["finite32"]:
            print("%s (no assertion): gpu-oracle32 %.3e gpu-oracle64 %.3e floor %.3e" % (tag, force_err(a, r["a32"]), force_err(a, r["a64"]), r["floor"]))
        if want_mode is not None:
            assert info.build_mode in want_mode
        assert info.warm_builds == 0
        first = tree_bits(eng)
        pv2, a2 = run_kd(eng, r["buf"], r["par"], n, fmm_order=p, unsort=1)
        again = eng.kd_info()
        print("%s again: build_mode %d, warm builds %d misses %d" % (tag, again.build_mode, again.warm_builds, again.warm_misses))
        assert_same_bits(first, tree_bits(eng), tag + " again")
        np.testing.assert_array_equal(bits(a2), bits(a))
        np.testing.assert_array_equal(bits(pv2), bits(pv))
        assert again.build_mode >= info.build_mode
    finally:
        eng.close()


# ---- B. warm rebuilds ------------------------------------------------------------------------------------------------------------
# every "forces" row that stays at two passes -- a context on three passes never selects warm -- and two "lists" rows, trees only:
# dup64 (64 candidates at every selection node, exactly what the resolver takes) and quant2048 (cut ties that the second key orders);
# test_the_warm_rows_are_the_rows_that_stay_at_two_passes holds this list against shapes3d.expected_mode
TREES_ONLY = ("dup64", "quant2048")
WARM_ROWS = [r for r in S.SELECT_CASES if r[3] == "forces" and r[0] != "ejected"] + [ROWS[(s, 20480, 4)] for s in TREES_ONLY]


def warm_rebuild(oracle32, oracle64, row):
    """three evaluations of a warm and a cold context with unsort = 0, tree_steps = 1 (see test_warm_rebuild_is_the_oracles_tree);
    returns the warm context's (warm_builds, warm_misses) after each, once per process"""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    if row in _warm:
        return _warm[row]
    shape, n, p, what = row
    tag = S.select_id(row)
    r = S.evaluate(oracle32, oracle64, S.kd_of(row))
    bound = S.force_bound(r["floor"]) if what == "forces" else None
    par = dev(r["par"])
    engines = [warm_engine(True, fmm_order=p, unsort=0, tree_steps=1), warm_engine(False, fmm_order=p, unsort=0, tree_steps=1)]
    states = [dev(r["buf"]), dev(r["buf"])]
    host = r["buf"][:2].copy()
    counts = []
    try:
        for k in range(3):
            if k == 2:
                for d in states:
                    d[0].mul_(1.001)
                host[0] *= np.float32(1.001)
            given = states[0][:2].cpu().numpy()
            np.testing.assert_array_equal(bits(given), bits(states[1][:2].cpu().numpy()))
            if k != 1:
                np.testing.assert_array_equal(bits(given), bits(host))          # (the fp32 multiply of the device is numpy's)
            buf = np.concatenate([given, np.zeros((1, n, 3), dtype=np.float32)])
            a, pv, t = S.run_oracle(oracle32, "kd", buf, r["par"], p, expansions=False, unsort=False)
            for name, e, d in zip(("warm", "cold"), engines, states):
                e.compute_force(EVAL_FMM_KDTREE, d, n, par, elastic=False)
                torch.cuda.synchronize()
                assert_oracle_tree(e, t, n, "%s evaluation %d %s" % (tag, k, name))
                got = d.cpu().numpy()
                np.testing.assert_array_equal(bits(got[:2]), bits(pv), err_msg="%s evaluation %d %s: state" % (tag, k, name))
                if bound is not None:
                    err = force_err(got[2], a)
                    print("%s evaluation %d %s: gpu-oracle32 %.3e bound %.3e" % (tag, k, name, err, bound))
                    if k < 2:          # (the case's floor is that of its own state, not of the stretched one)
                        assert err < bound
            assert torch.equal(states[0].view(torch.int32), states[1].view(torch.int32)), "%s evaluation %d: warm != cold" % (tag, k)
            assert_same_bits(tree_bits(engines[0]), tree_bits(engines[1]), "%s evaluation %d: warm != cold" % (tag, k))
            iw, ic = engines[0].kd_info(), engines[1].kd_info()
            print("%s evaluation %d: warm_builds %d warm_misses %d build_mode %d (cold context: %d)"
                  % (tag, k, iw.warm_builds, iw.warm_misses, iw.build_mode, ic.build_mode))
            assert ic.warm_builds == 0 and ic.warm_misses == 0
            counts.append((iw.warm_builds, iw.warm_misses, iw.build_mode))
            host = pv.copy()
    finally:
        for e in engines:
            e.close()
    _warm[row] = counts
    return counts


@pytest.mark.parametrize("row", WARM_ROWS, ids=S.select_id)
def test_warm_rebuild_is_the_oracles_tree(oracle32, oracle64, row):
    """A context that rebuilds warm and one that never does, three evaluations each: the state as given; the tree-ordered state it
    left (the warm select is handed its own pivots back: a warm build, and no miss); that state stretched by 1.001 (pivots 1e-3 of
    a box away from the medians: a miss is allowed, and repeated cold).  Before every evaluation the state is downloaded and given
    to the fp32 oracle (unsort = 0): tree, permutation, lists and the tree-ordered positions and velocities of BOTH contexts are the
    oracle's, and the two contexts are bit-equal in state, accelerations and tree.  dup64 (NaN forces in the reference) and
    quant2048 (lists that differ between the two oracles) are compared in trees and state only."""
    assert (row[3] == "forces" and S.expected_mode(oracle32, oracle64, row) == {0}) or row[0] in TREES_ONLY, "not a row of this test"
    counts = warm_rebuild(oracle32, oracle64, row)
    assert counts[0][:2] == (0, 0)          # nothing to select around yet
    if row[0] != "dup64":
        assert counts[1][:2] == (1, 0) and counts[1][2] == 0
    assert counts[2][0] >= counts[1][0] and counts[2][1] <= counts[1][1] + 1


def test_a_tied_row_took_the_warm_tie_path(oracle32, oracle64):
    """8 and 16 copies of every point: the warm select's candidates are tied in their first key and ordered by the second, the
    third and the original index.  At least one of the two rows has to have done that in a warm build that did not miss."""
    hits = [row for row in TIED if warm_rebuild(oracle32, oracle64, row)[1][:2] == (1, 0)]
    print("warm builds through exact ties:", [S.select_id(r) for r in hits])
    assert hits


def test_the_warm_rows_are_the_rows_that_stay_at_two_passes(oracle32, oracle64):
    want = [r for r in S.SELECT_CASES if (r[3] == "forces" and S.expected_mode(oracle32, oracle64, r) == {0}) or r[0] in TREES_ONLY]
    assert sorted(want) == sorted(WARM_ROWS) and set(TIED) <= set(WARM_ROWS)


# ---- C. a fused run --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", FUSED, ids=S.select_id)
def test_fused_steps_on_a_degenerate_shape_equal_step_by_step(oracle32, row):
    """four leapfrog steps as ONE nbco_integrate_steps call on a warm context (the pass between two steps does the next build's
    prologue) against four nbco_integrate calls on a cold one: state, accelerations, tree and pair counts bit-equal"""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    shape, n, p, _ = row
    steps, dt = 4, 5e-4
    buf = S.state(oracle32, shape, n)
    par = dev(oracle32.params(n))
    out = []
    for warm in (True, False):
        e = warm_engine(warm, fmm_order=p, unsort=0, tree_steps=1)
        d = dev(buf)
        e.compute_force(EVAL_FMM_KDTREE, d, n, par, elastic=True)
        if warm:
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, par, dt, steps, elastic=True)
        else:
            for _ in range(steps):
                e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, par, dt, elastic=True)
        torch.cuda.synchronize()
        info = e.kd_info()
        print("%s %s: warm_builds %d warm_misses %d build_mode %d, %d leaf pairs, %d M2L pairs"
              % (S.select_id(row), "fused warm" if warm else "stepwise cold", info.warm_builds, info.warm_misses, info.build_mode, info.p2p_pairs, info.m2l_pairs))
        out.append((d.cpu().numpy(), tree_bits(e)))
        e.close()
    assert np.isfinite(out[0][0]).all()
    np.testing.assert_array_equal(bits(out[0][0]), bits(out[1][0]))
    assert_same_bits(out[0][1], out[1][1], S.select_id(row))
